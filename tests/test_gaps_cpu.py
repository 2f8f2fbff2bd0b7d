"""CPU: the host side of the absence runs — the numpy restatement of k_absence_runs (tests/gaps_ref.py) against a hand-written
loop, panagram_amd/gaps.py (join_pieces, classify, the frames), the run-length arithmetic pinned on rows the oracle computes
from planted variants, and Genome.absence_runs / the `gaps` subcommand over test_pair_counts_cpu.py's in-memory index with a
numpy stand-in for the rows container."""
import os
import re

import numpy as np
import pandas as pd
import pytest

from panagram_amd import gaps
from tests import gaps_ref as gr
from tests import rows_craft as rc
from tests.test_pair_counts_cpu import LOW, REGIONS, SIZES, _scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------
# the restatement against a loop
# ---------------------------------------------------------------------------
def _loop(bits, maxlen):
    """row by row, column by column: the same four results"""
    m, n = bits.shape
    runs, hist, absent, edges = [], np.zeros((n, maxlen + 1), np.int64), np.zeros(n, np.int64), np.zeros((n, 2), np.int64)
    for g in range(n):
        length, seen = 0, False
        for j in range(m):
            if bits[j, g]:
                if length and seen:
                    runs.append((g, j - length, length))
                    hist[g, min(length, maxlen)] += 1
                elif length:
                    edges[g, 0] = length
                seen, length = True, 0
            else:
                length += 1
                absent[g] += 1
        edges[g, 1] = length
        if not seen:
            edges[g, 0] = length
    return np.array(runs, np.int64).reshape(-1, 3), hist, absent, edges


def _same(got, want, tag):
    for a, b, what in zip(got, want, ("runs", "hist", "absent", "edges")):
        assert np.array_equal(np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)), (tag, what)


def _column(pattern):
    return np.array([[int(c)] for c in pattern], np.uint8)


@pytest.mark.parametrize("pattern, runs, head, tail", [
    ("1001110001", [(1, 2), (6, 3)], 0, 0),
    ("0011000", [], 2, 3),            # open on both sides, nothing closed
    ("0000", [], 4, 4),               # absent throughout: both edges the window
    ("1111", [], 0, 0),
    ("", [], 0, 0),                   # an empty window
    ("0", [], 1, 1),
    ("1", [], 0, 0),
    ("0101", [(2, 1)], 1, 0),
    ("10", [], 0, 1),
])
def test_reference_on_a_dozen_rows(pattern, runs, head, tail):
    got = gr.ref_window(_column(pattern).reshape(len(pattern), 1), 3)
    assert [tuple(r[1:]) for r in got[0].tolist()] == runs and got[3].tolist() == [[head, tail]]
    assert got[2].tolist() == [pattern.count("0")]
    assert got[1][0].tolist() == np.bincount([min(b, 3) for _, b in runs], minlength=4).tolist()
    _same(got, _loop(_column(pattern).reshape(len(pattern), 1), 3), pattern)


def test_reference_equals_the_loop():
    rng = np.random.default_rng(11)
    for n, m, density, maxlen in [(1, 300, 0.5, 4), (9, 500, 0.9, 21), (33, 257, 0.1, 1), (5, 64, 0.5, 4096), (3, 0, 0.5, 5)]:
        bits = (rng.random((m, n)) < density).astype(np.uint8)
        if m:
            bits[:, n - 1] = 0  # a column absent throughout
        _same(gr.ref_window(bits, maxlen), _loop(bits, maxlen), (n, m, maxlen))
    # windows, strides, the selection and the length filter of ref_absence_runs
    rows = [rc.with_pad_bits(rc.dense(400, 11, 3), 11), rc.dense(90, 11, 4)]
    for stride in (1, 3):
        c, s, e = [0, 1, 0, 0], [0, 2, 17, 5], [(400 - 1) // stride + 1, 20, 18, 5]
        got = gr.ref_absence_runs(rows, 11, c, s, e, stride, 6, min_len=2, max_len=3, cols=[0, 4, 10])
        for i in range(4):
            bits = rc.unpack(rows[c[i]][::stride], 11)[s[i]:e[i]].copy()
            bits[:, [g for g in range(11) if g not in (0, 4, 10)]] = 1  # unselected: nothing absent, nothing counted
            r, h, a, ed = _loop(bits, 6)
            r = r[(r[:, 2] >= 2) & (r[:, 2] <= 3)] + np.array([0, s[i], 0])
            _same((got[0][got[0][:, 0] == i][:, 1:], got[1][i], got[2][i], got[3][i]), (r, h, a, ed), (stride, i))
        assert len(got[0]) > 10 and np.array_equal(got[0], got[0][np.lexsort((got[0][:, 2], got[0][:, 1], got[0][:, 0]))])


# ---------------------------------------------------------------------------
# gaps.py
# ---------------------------------------------------------------------------
def _crafted_bits():
    """120 rows of 6 genomes: column 0 one run [30, 70), column 1 runs that end / begin at rows the cuts fall on, column 2
    absent throughout, column 3 present throughout, column 4 open runs at both edges and a row-long run, column 5 dense"""
    bits = np.ones((120, 6), np.uint8)
    bits[30:70, 0] = 0
    bits[28:31, 1] = 0
    bits[33:69, 1] = 0
    bits[71:73, 1] = 0
    bits[:, 2] = 0
    bits[:29, 4] = 0
    bits[50, 4] = 0
    bits[68:, 4] = 0
    bits[:, 5] = np.random.default_rng(2).random(120) < 0.5
    return bits


@pytest.mark.parametrize("npieces", [2, 3, 7])
@pytest.mark.parametrize("min_len, max_len, maxlen", [(1, 0, 84), (2, 39, 5), (40, 40, 40)])
def test_join_pieces_equals_the_uncut_window(npieces, min_len, max_len, maxlen):
    bits = _crafted_bits()
    want = gr.ref_window(bits, maxlen)
    keep = (want[0][:, 2] >= min_len) & ((want[0][:, 2] <= max_len) if max_len else True)
    want = (want[0][keep],) + want[1:]
    throughout = 0
    for x in list(range(26, 36)) + list(range(66, 76)):  # every offset near the ends of the runs of columns 0, 1 and 4
        cuts = [0] + [x + 3 * i for i in range(npieces - 1)] + [120]  # (pieces of 3 rows behind the first cut)
        pieces = []
        for p0, p1 in zip(cuts[:-1], cuts[1:]):
            r, h, a, ed = gr.ref_window(bits[p0:p1], maxlen)
            r = r[(r[:, 2] >= min_len) & ((r[:, 2] <= max_len) if max_len else True)]
            pieces.append((p0, p1 - p0, r, h, a, ed))
            throughout += int(ed[0, 0] == p1 - p0)
        _same(gaps.join_pieces(pieces, 6, maxlen, min_len, max_len), want, (npieces, x))
    assert npieces == 2 or throughout >= 8  # pieces that column 0 is absent from throughout (3 pieces: the 8 cuts 30..35, 66, 67)
    # no piece, and one piece
    _same(gaps.join_pieces([], 6, maxlen), (np.zeros((0, 3)), np.zeros((6, maxlen + 1)), np.zeros(6), np.zeros((6, 2))), "none")
    one = gr.ref_window(bits, maxlen)
    _same(gaps.join_pieces([(0, 120) + one], 6, maxlen), one, "one")


def test_join_pieces_on_random_rows_at_every_piece_length():
    bits = (np.random.default_rng(8).random((500, 9)) < 0.4).astype(np.uint8)
    bits[100:400, 8] = 0
    want = gr.ref_window(bits, 30)
    for per in (1, 2, 7, 100, 499, 500, 5000):
        pieces = [(p0, len(bits[p0:p0 + per])) + gr.ref_window(bits[p0:p0 + per], 30) for p0 in range(0, 500, per)]
        _same(gaps.join_pieces(pieces, 9, 30), want, per)
    with pytest.raises(ValueError, match="shapes"):
        gaps.join_pieces([(0, 500) + gr.ref_window(bits, 31)], 9, 30)


def test_classify():
    k = 21
    cls, site, span = gaps.classify([k, k - 1, k + 1, k - 2, 1, 3 * k], k, start=[100, 200, 300, 400, 500, 600])
    assert cls.tolist() == ["sub", "ins", "del_or_multi", "short", "short", "del_or_multi"]
    assert site.tolist() == [120, 220, 320, -1, -1, 620] and span.tolist() == [1, 0, 2, 0, 0, 2 * k + 1]
    cls, site, span = gaps.classify([k, 5], k, start=7, open=True)  # an open run has no class, whatever its length
    assert cls.tolist() == ["open", "open"] and site.tolist() == [-1, -1] and span.tolist() == [0, 0]
    assert set(cls.tolist()) | {"sub", "ins", "del_or_multi", "short"} == set(gaps.CLASSES)
    cls, site, span = gaps.classify(k, k, 9)
    assert cls.item() == "sub" and site.item() == 9 + k - 1 and span.item() == 1
    with pytest.raises(ValueError):
        gaps.classify([3], 1)


def test_select_words_and_length_checks():
    names = [f"g{i}" for i in range(70)]
    words, sel = gaps.select_words(names)
    assert sel == names and np.array_equal(words, rc.words_of(70, range(70)))  # (more than 64 genomes: no limit here)
    words, sel = gaps.select_words(names, ["g69", 3, "g32"])
    assert sel == ["g3", "g32", "g69"] and np.array_equal(words, rc.words_of(70, [3, 32, 69])) and words.dtype == np.uint32
    for bad, msg in [(["zz"], "'zz'"), ([70], "out of range"), (["g1", 1], "twice"), ([], "no genome")]:
        with pytest.raises(ValueError, match=msg):
            gaps.select_words(names, bad)
    gaps.check_lengths(1, 1, 0)
    gaps.check_lengths(4096, 5, 3)
    for bad in [(0, 1, 0), (4097, 1, 0), (5, 0, 0), (5, 1, -1)]:
        with pytest.raises(ValueError):
            gaps.check_lengths(*bad)


def test_spectrum_and_summary_frames():
    k, maxlen = 5, 8
    bits = np.ones((200, 3), np.uint8)
    for a, b in [(10, 15), (20, 24), (30, 37), (50, 59), (70, 82), (100, 105)]:  # 5, 4, 7, 9, 12, 5 rows
        bits[a:b, 1] = 0
    bits[:3, 1] = 0
    bits[190:, 1] = 0
    bits[:, 2] = 0
    runs, hist, absent, edges = gr.ref_window(bits, maxlen)
    names = ["a", "b", "c"]
    sp = gaps.spectrum_frame(hist, names)
    assert list(sp.columns) == ["genome", "rows", "runs"]
    assert sp.values.tolist() == [["b", 4, 1], ["b", 5, 2], ["b", 7, 1], ["b", 8, 2]]  # (9 and 12 rows: the last bin)
    su = gaps.summary_frame(hist, absent, gaps.open_rows(edges, 200), 200, names, k)
    assert list(su.columns) == ["genome", "rows", "absent", "runs", "sub", "ins", "del_or_multi", "long_rows", "sub_per_kb"]
    assert su.loc[1].tolist() == ["b", 200, 42 + 13, 6, 2, 1, 3, 21, 10.0]
    assert su.loc[0].tolist()[1:] == [200, 0, 0, 0, 0, 0, 0, 0.0]
    assert su.loc[2].tolist()[1:] == [200, 200, 0, 0, 0, 0, 0, 0.0]  # absent throughout: 200 open rows, counted once
    with pytest.raises(ValueError, match="past k"):
        gaps.summary_frame(hist[:, :k + 1], absent, gaps.open_rows(edges, 200), 200, names, k)
    # the invariant the GPU test holds the kernel to
    short = (hist[:, :maxlen] * np.arange(maxlen)).sum(axis=1)
    capped = np.array([sum(r[2] for r in runs.tolist() if r[0] == g and r[2] >= maxlen) for g in range(3)])
    assert np.array_equal(short + capped + gaps.open_rows(edges, 200), absent)


# ---------------------------------------------------------------------------
# the interpretation, pinned on rows the oracle computes
# ---------------------------------------------------------------------------
def test_planted_variants_give_the_runs_the_arithmetic_says():
    from oracle import pyoracle as po
    k = gr.PLANTED_K
    a, b = gr.planted_genomes()
    # the seed's own conditions: the deleted bases 1400..1402 can be shifted neither way
    assert a[1400] != a[1403] and a[1399] != a[1402]
    A, B = po.codes_to_ascii(a), po.codes_to_ascii(b)
    rows = po.anchor_contig(po.build_bitvec_dbs([[A], [B]], k), A, k, 2)[0]
    bits = rc.unpack(rows, 2)
    assert len(bits) == gr.PLANTED_LEN - k + 1
    runs, hist, absent, edges = gr.ref_window(bits, 4 * k)
    # the anchor's own column and the flanks hold no absent row: no chance repeat hides behind the four runs
    assert absent[0] == 0 and not edges.any()
    planted = np.zeros(len(bits), bool)
    for s, n, *_ in gr.PLANTED_RUNS:
        planted[s:s + n] = True
    assert bits[~planted, 1].all()
    assert runs.tolist() == [[1, s, n] for s, n, *_ in gr.PLANTED_RUNS]
    assert absent[1] == 21 + 28 + 23 + 20
    cls, site, span = gaps.classify(runs[:, 2], k, runs[:, 1])
    assert list(zip(cls.tolist(), site.tolist(), span.tolist())) == [r[2:] for r in gr.PLANTED_RUNS]
    su = gaps.summary_frame(hist, absent, gaps.open_rows(edges, len(bits)), len(bits), ["a", "b"], k)
    assert su.loc[1, ["runs", "sub", "ins", "del_or_multi", "long_rows"]].tolist() == [4, 1, 1, 2, 0]


# ---------------------------------------------------------------------------
# Genome.absence_runs / absence_spectrum and the subcommand over an in-memory index
# ---------------------------------------------------------------------------
class _Rows:
    """stands in for a rows container of one contig: what k_absence_runs would return, by tests/gaps_ref.py"""

    def __init__(self, rows, n, bstep):
        self.rows, self.n, self.bstep = rows, n, bstep

    def absence_runs(self, contigs, starts, ends, select_words=None, maxlen=84, min_len=1, max_len=0, step=1, stride=1, emit=True):
        assert step == self.bstep and list(contigs) == [0] * len(starts)
        for e in ends:
            assert e == 0 or (int(e) - 1) * stride < len(self.rows)  # every sampled row inside the contig
        cols = None if select_words is None else np.flatnonzero(rc.keep_bits(self.n, select_words)).tolist()
        runs, hist, absent, edges = gr.ref_absence_runs([self.rows], self.n, contigs, starts, ends, stride, maxlen, min_len, max_len, cols)
        return (runs if emit else runs[:0]), hist.astype(np.uint64), absent.astype(np.uint64), edges.astype(np.uint64)

    def close(self):
        pass


def _gaps_scene(monkeypatch, n, k=5):
    idx, g, log = _scene(monkeypatch, n, density=0.8)
    idx.k, g.anchored = k, True
    region = g._rows_region
    g._rows_region = lambda bstep, row0, nrows: _Rows(region(bstep, row0, nrows).rows, n, bstep)
    return idx, g, log


def _want_frame(g, k, genomes, chrom, start, end, step, min_len, max_len):
    parts = []
    for c in (list(SIZES) if chrom is None else [chrom]):
        frame = g.query(c, start, end, step)
        labels = frame.index.to_numpy().astype(np.int64)
        names = list(frame.columns)
        runs = gr.ref_window(frame.to_numpy(), 1, [names.index(x) for x in genomes] if genomes else None)[0]
        runs = runs[(runs[:, 2] >= min_len) & ((runs[:, 2] <= max_len) if max_len else True)]
        runs = runs[np.lexsort((runs[:, 0], runs[:, 1]))]
        cls, site, _ = gaps.classify(runs[:, 2], k, labels[runs[:, 1]] if len(runs) else 0)
        parts.append(pd.DataFrame({"chr": np.full(len(runs), c, object), "start": labels[runs[:, 1]] if len(runs) else [],
                                   "end": labels[runs[:, 1] + runs[:, 2] - 1] + 1 if len(runs) else [],
                                   "genome": [names[i] for i in runs[:, 0]], "rows": runs[:, 2],
                                   "class": cls if step == 1 else [""] * len(runs), "site": site if step == 1 else [-1] * len(runs)}))
    return pd.concat(parts, ignore_index=True)


def _same_frame(got, want, tag):
    assert list(got.columns) == ["chr", "start", "end", "genome", "rows", "class", "site"] and len(got) == len(want), (tag, len(got), len(want))
    for col in ("chr", "genome", "class"):
        assert got[col].tolist() == want[col].tolist(), (tag, col)
    for col in ("start", "end", "rows", "site"):
        assert np.array_equal(got[col].to_numpy().astype(np.int64), want[col].to_numpy().astype(np.int64)), (tag, col)


@pytest.mark.parametrize("step", [1, 7, 100, 300])
def test_absence_runs_selects_and_labels_querys_rows(monkeypatch, step):
    idx, g, log = _gaps_scene(monkeypatch, 11)
    total = 0
    for genomes, min_len, max_len in [(None, 1, 0), (["g3", "g10"], 2, 6)]:
        for chrom, start, end in REGIONS + [(None, None, None)]:
            got = g.absence_runs(genomes, chrom, start, end, step, min_len, max_len)
            _same_frame(got, _want_frame(g, 5, genomes, chrom, start, end, step, min_len, max_len), (genomes, chrom, start, end, step))
            _same_frame(idx.absence_runs("g0", genomes, chrom, start, end, step, min_len, max_len), got, "Index.absence_runs")
            total += len(got)
    assert total > (20 if step < LOW else 5)  # (the low-resolution steps leave a dozen rows per region)


@pytest.mark.parametrize("step,rows_per_piece", [(7, 50), (1, 97), (300, 5), (1, 1)])
def test_tiny_budget_never_cuts_a_run(monkeypatch, step, rows_per_piece):
    idx, g, log = _gaps_scene(monkeypatch, 11)
    bstep = LOW if step % LOW == 0 else 1
    whole = g.absence_tables(None, "c1", 3, 1230, step, maxlen=6)
    n0 = len(log)
    g.similarity_budget = rows_per_piece * g.nbytes * bstep
    cut = g.absence_tables(None, "c1", 3, 1230, step, maxlen=6)
    assert len(log) - n0 >= 3 and all(nrows <= rows_per_piece for _, _, nrows in log[n0:])
    _same_frame(cut[0], whole[0], (step, rows_per_piece))
    _same_frame(whole[0], _want_frame(g, 5, None, "c1", 3, 1230, step, 1, 0), "uncut")
    assert cut[1].equals(whole[1]) and (step != 1 or cut[2].equals(whole[2]))
    frame = g.query("c1", 3, 1230, step)
    want = gaps.spectrum_frame(gr.ref_window(frame.to_numpy(), 6)[1], list(frame.columns))
    assert whole[1].equals(want) and g.absence_spectrum(None, "c1", 3, 1230, step, 6).equals(want)
    assert idx.absence_spectrum("g0", None, "c1", 3, 1230, step, 6).equals(want)


def test_absence_input_errors(monkeypatch):
    idx, g, log = _gaps_scene(monkeypatch, 3)
    with pytest.raises(KeyError, match="no chromosome"):
        g.absence_runs(chrom="nope")
    with pytest.raises(ValueError, match="need a chromosome"):
        g.absence_runs(start=5, end=10)
    with pytest.raises(ValueError, match="'nobody'"):
        g.absence_runs(["nobody"])
    with pytest.raises(ValueError):
        g.absence_runs(min_len=0)
    with pytest.raises(ValueError, match="maxlen"):
        g.absence_spectrum(maxlen=5000)
    assert log == []  # nothing was read


def test_cli_gaps(monkeypatch, tmp_path, capsys):
    from panagram_amd import index as pidx
    from panagram_amd.__main__ import main
    idx, g, log = _gaps_scene(monkeypatch, 9)
    monkeypatch.setattr(pidx, "Index", lambda path, mode=None, device=0: idx)
    out, sp, su = tmp_path / "runs.tsv", tmp_path / "sp.tsv", tmp_path / "su.tsv"
    assert main(["gaps", "some/index", "g0", "c1", "13", "1001", "-o", str(out), "--spectrum", str(sp), "--summary", str(su)]) == 0
    want = g.absence_tables(None, "c1", 13, 1001, 1, 4, 0, 20)  # (the defaults: min_len = k - 1, maxlen = 4 k)
    assert len(want[0]) > 5 and want[0]["rows"].min() == 4
    got = pd.read_csv(out, sep="\t", header=None, names=list(want[0].columns))
    _same_frame(got, want[0], "-o")
    assert pd.read_csv(sp, sep="\t").equals(want[1]) and len(want[1]) > 9
    got = pd.read_csv(su, sep="\t")
    assert list(got.columns) == list(want[2].columns) and np.allclose(got.iloc[:, 1:].to_numpy(), want[2].iloc[:, 1:].to_numpy().astype(float))
    # stdout, the whole genome, a selection and the length filter
    assert main(["gaps", "some/index", "g0", "--whole", "--genomes", "g2,g5", "--min-len", "2", "--max-len", "3"]) == 0
    lines = [ln.split("\t") for ln in capsys.readouterr().out.splitlines()]
    want = g.absence_runs(["g2", "g5"], None, None, None, 1, 2, 3)
    assert len(want) > 5 and [ln[:5] for ln in lines] == [[str(v) for v in row[:5]] for row in want.values.tolist()]
    for bad in (["gaps", "some/index", "g0"], ["gaps", "some/index", "g0", "c1", "--whole"], ["gaps", "some/index", "g0", "c1", "--genomes", "nobody"],
                ["gaps", "some/index", "g0", "c1", "--summary", str(su), "--maxlen", "5"]):
        with pytest.raises(SystemExit):
            main(bad)


def test_chunk_constant_is_the_kernels():
    from panagram_amd import engine
    txt = open(os.path.join(ROOT, "panagram_amd", "csrc", "pg_kernels.h")).read()
    assert int(re.search(r"constexpr uint32_t GAPS_CHUNK = (\d+);", txt).group(1)) == engine.GAPS_CHUNK
    assert engine.GAPS_CHUNK % 256 == 0 and engine.GAPS_FIRST_CAP > 0
