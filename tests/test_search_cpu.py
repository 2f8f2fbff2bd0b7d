"""CPU: the host side of search — the numpy model of the presence profile (tests/search_ref.py) against a hand-written loop that
marks bases, against the two identities of include/panagram_hip.h (pg_result_presence_profile) and against tests/gaps_ref.py on
the same matrices; panagram_amd/search.py's FASTA scan, batching and frames; the `search` subcommand's argument errors; and
tools/profile_stitch_check.cpp, compiled without sanitizer flags and run."""
import os
import re
import shutil
import subprocess

import numpy as np
import pandas as pd
import pytest

from panagram_amd import search
from panagram_amd.index import Index as _RealIndex
from tests import gaps_ref as gr
from tests import search_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _loop(p, k):
    """the six fields of one column by the definitions, row by row, marking every base of every held k-mer"""
    n = len(p)
    base = [0] * (n + k - 1)
    hits = runs = longest = first = end = run = 0
    for i, v in enumerate(p):
        if not v:
            run = 0
            continue
        if hits == 0:
            first = i
        hits += 1
        run += 1
        runs += run == 1
        longest = max(longest, run)
        end = i + 1
        for b in range(i, i + k):
            base[b] = 1
    return [hits, runs, longest, first, end, sum(base)]


def _vectors(rng, count, nmax):
    for t in range(count):
        n = int(rng.integers(0, nmax + 1))
        kind = t % 5
        if kind == 0:
            p = rng.random(n) < rng.random()
        elif kind == 1:  # long runs and long gaps
            p = np.cumsum(rng.random(n) < 0.05) % 2 == 0
        elif kind == 2:
            p = rng.random(n) < 0.03
        elif kind == 3:
            p = rng.random(n) < 0.97
        else:
            p = np.full(n, t % 2 == 0)
        yield p.astype(np.uint8)


def test_model_equals_the_loop_and_both_identities():
    rng = np.random.default_rng(1)
    seen_gap = set()
    for t, p in enumerate(_vectors(rng, 3000, 200)):
        k = 1 + t % 32
        got, (every, none) = sr.ref_window(p[:, None], k)
        want = _loop(p.tolist(), k)
        assert got.tolist() == [want], (t, k, p.tolist())
        assert (every, none) == (int(p.sum()), int(len(p) - p.sum()))
        hits, runs, longest, first, end, covered = want
        gaps = sr.gap_lengths(p)
        assert covered == hits + int(np.minimum(gaps, k - 1).sum()) + (k - 1 if hits else 0), (t, k)
        assert runs == len(gaps) + (1 if hits else 0), (t, k)
        assert covered <= max(0, len(p) + k - 1) and longest <= hits and (hits == 0 or first < end)
        seen_gap |= {int(g) - k for g in gaps if abs(int(g) - k) <= 2}
    assert seen_gap == {-2, -1, 0, 1, 2}  # gaps of k - 2 .. k + 2 rows occurred


def test_model_selection_windows_and_rows():
    rng = np.random.default_rng(2)
    bits = (rng.random((300, 11)) < 0.6).astype(np.uint8)
    bits[40:90, 3] = 1
    bits[:, 7] = 0
    k = 5
    full, (every, none) = sr.ref_window(bits, k)
    assert full[:, :].tolist() == [_loop(bits[:, g].tolist(), k) for g in range(11)]
    assert every == 0 and none == int((bits.sum(axis=1) == 0).sum())
    cols = [0, 3, 10]
    part, (every, none) = sr.ref_window(bits, k, cols)
    assert np.array_equal(part[cols], full[cols]) and not np.delete(part, cols, axis=0).any()
    assert every == int(bits[:, cols].all(axis=1).sum()) and none == int((~bits[:, cols].any(axis=1)).sum()) and every > 0
    for empty in (sr.ref_window(bits, k, []), sr.ref_window(bits[:0], k)):
        assert not empty[0].any() and empty[1] == (0, 0)
    from tests import rows_craft as rc
    rows = [rc.with_pad_bits(rc.pack(bits), 11), rc.pack(bits[::-1])]
    prof, allnone = sr.ref_presence_profile(rows, 11, k, [0, 1, 0, 1], [0, 0, 17, 5], [300, 300, 17, 205], cols)
    assert np.array_equal(prof[0], part) and np.array_equal(prof[1], sr.ref_window(bits[::-1], k, cols)[0])
    assert not prof[2].any() and allnone[2].tolist() == [0, 0]
    assert np.array_equal(prof[3], sr.ref_window(bits[::-1][5:205], k, cols)[0])


def test_model_agrees_with_the_absence_runs_reference():
    """on the same matrices: hits = n - absent; first and end from the open runs at the edges; the clipped gap sum from the
    spectrum of closed runs"""
    rng = np.random.default_rng(3)
    for t in range(40):
        n, N, k = int(rng.integers(1, 400)), int(rng.integers(1, 20)), 1 + t % 32
        bits = (rng.random((n, N)) < rng.random(N)[None, :]).astype(np.uint8)
        if t % 4 == 0:
            bits[:, 0] = 0
        cols = None if t % 3 else sorted(set(rng.integers(0, N, 3).tolist()))
        prof, _ = sr.ref_window(bits, k, cols)
        maxlen = 40
        runs, hist, absent, edges = gr.ref_window(bits, maxlen, cols)
        sel = range(N) if cols is None else cols
        for g in sel:
            hits, nruns, longest, first, end, covered = prof[g].tolist()
            assert hits == n - absent[g]
            if hits:
                assert first == edges[g, 0] and end == n - edges[g, 1]
                assert nruns == hist[g].sum() + 1
                assert covered == hits + int((hist[g] * np.minimum(np.arange(maxlen + 1), k - 1)).sum()) + k - 1
            else:
                assert edges[g].tolist() == [n, n] and [first, end, nruns, covered] == [0, 0, 0, 0]


# ---------------------------------------------------------------------------
# panagram_amd/search.py
# ---------------------------------------------------------------------------
def test_scan_fasta_follows_the_packers_rules():
    text = b"ignored\n>a some words\nACGT\nAC\n>b\n\n>  c\tx\r\nAC GT\r\nN\n>a\nacgtn>x\n>last"
    names, lens, offs = search.scan_fasta(text)
    assert names == ["a", "b", "c", "a", "last"] and lens.tolist() == [6, 0, 5, 7, 0]
    assert [bytes(text[offs[i]:offs[i + 1]])[:2] for i in range(5)] == [b">a", b">b", b"> ", b">a", b">l"] and offs[-1] == len(text)
    for empty in (b"", b"no header\nACGT\n"):
        names, lens, offs = search.scan_fasta(empty)
        assert names == [] and len(lens) == 0 and offs.tolist() == [len(empty)]
    names, lens, offs = search.scan_fasta(np.frombuffer(b">only\nAC", np.uint8))
    assert names == ["only"] and lens.tolist() == [2]
    text, names, lens, offs = search.read_queries([("q1", "ACGT"), ("q1", b"AC\nGT\nA"), ("q3", "")])
    assert names == ["q1", "q1", "q3"] and lens.tolist() == [4, 5, 0]
    for bad in ([("two words", "AC")], [("", "AC")], [("q", "AC>GT")]):
        with pytest.raises(ValueError):
            search.read_queries(bad)


def test_read_queries_from_files(tmp_path):
    import gzip
    fa = b">x\nACGT\nAC\n>y\nA\n"
    (tmp_path / "q.fa").write_bytes(fa)
    with gzip.open(tmp_path / "q.fa.gz", "wb") as f:
        f.write(fa)
    for src in (str(tmp_path / "q.fa"), tmp_path / "q.fa.gz", fa, bytearray(fa)):
        text, names, lens, offs = search.read_queries(src)
        assert names == ["x", "y"] and lens.tolist() == [6, 1] and bytes(text) == fa


def test_batches():
    assert search.batches([], 10) == []
    assert search.batches([3], 10) == [(0, 1)]
    assert search.batches([5, 5, 5, 20, 1, 1], 10) == [(0, 2), (2, 3), (3, 4), (4, 6)]  # exact fits, an oversize record alone
    assert search.batches([10, 1, 9, 0, 0, 11], 10) == [(0, 1), (1, 5), (5, 6)]
    assert search.batches([4, 4, 4], 1) == [(0, 1), (1, 2), (2, 3)]
    assert search.batches([4, 4, 4], search.BATCH_BASES) == [(0, 3)] and search.BATCH_BASES == 1 << 26
    lens = np.random.default_rng(4).integers(0, 50, 500)
    got = search.batches(lens, 120)
    assert got[0][0] == 0 and got[-1][1] == 500 and all(a[1] == b[0] for a, b in zip(got, got[1:]))
    assert all(lens[i:j].sum() <= 120 or j == i + 1 for i, j in got)
    assert all(lens[i:j + 1].sum() > 120 for i, j in got[:-1])  # no batch could have taken the next record
    with pytest.raises(ValueError):
        search.batches([1], 0)


def _hand_made():
    """four queries (a duplicate name, one shorter than k) x three genomes at k = 5"""
    names, lens, k = ["q", "short", "q", "none"], [14, 4, 24, 9], 5
    prof = np.zeros((4, 3, 6), np.uint32)
    prof[0, 0] = [10, 1, 10, 0, 10, 14]   # whole
    prof[0, 1] = [5, 1, 5, 0, 5, 9]       # one substitution at base 9: the first five k-mers are left
    prof[0, 2] = [10, 1, 10, 0, 10, 14]   # whole as well: a tie with g0
    prof[2, 1] = [10, 2, 5, 0, 20, 18]    # kmers = 20: half of them, 18 of 24 bases
    prof[2, 2] = [12, 3, 6, 2, 19, 17]    # more k-mers, fewer bases
    rows = np.array([[5, 0], [0, 0], [8, 6], [0, 5]], np.uint32)
    return names, lens, k, ["g0", "g1", "g2"], prof, rows


def test_frames_from_hand_made_profiles():
    names, lens, k, genomes, prof, rows = _hand_made()
    long, matrix, summary = search.frames(names, lens, k, genomes, prof, rows)
    assert list(long.columns) == search.LONG_COLUMNS and len(long) == 12
    assert long["query"].tolist() == [n for n in names for _ in range(3)] and long["genome"].tolist() == genomes * 4
    assert long["length"].tolist() == [n for n in lens for _ in range(3)]
    assert long["kmers"].tolist() == [10] * 3 + [0] * 3 + [20] * 3 + [5] * 3
    assert long["frac"].tolist() == [1.0, 0.5, 1.0, 0, 0, 0, 0, 0.5, 0.6, 0, 0, 0]
    assert np.allclose(long["cov_frac"], [1.0, 9 / 14, 1.0, 0, 0, 0, 0, 0.75, 17 / 24, 0, 0, 0])
    for i, name in enumerate(search.FIELDS):
        assert long[name].tolist() == prof[:, :, i].ravel().tolist()
    # a query shorter than k: zeros, not a division by zero
    short = long[long["query"] == "short"]
    assert len(short) == 3 and not short[["kmers", "hits", "frac", "covered", "cov_frac"]].to_numpy().any()
    assert np.isfinite(long[["frac", "cov_frac"]].to_numpy()).all()
    assert matrix.index.tolist() == names and list(matrix.columns) == genomes and matrix.index.name == "query"
    assert matrix.to_numpy().tolist() == [[1.0, 0.5, 1.0], [0, 0, 0], [0, 0.5, 0.6], [0, 0, 0]]
    assert list(summary.columns) == search.SUMMARY_COLUMNS and summary["query"].tolist() == names
    assert summary["all"].tolist() == [5, 0, 8, 0] and summary["none"].tolist() == [0, 0, 6, 5]
    assert summary["genomes_hit"].tolist() == [3, 0, 2, 0]
    assert summary["best"].tolist() == ["g0", "-", "g2", "-"]  # (the tie of g0 and g2: genome order)
    assert summary["best_frac"].tolist() == [1.0, 0.0, 0.6, 0.0]
    # by bases: cov_frac decides the matrix, best and --min-frac
    long_b, matrix_b, summary_b = search.frames(names, lens, k, genomes, prof, rows, 0.72, "bases")
    assert np.allclose(matrix_b.to_numpy(), [[1.0, 9 / 14, 1.0], [0, 0, 0], [0, 0.75, 17 / 24], [0, 0, 0]])
    assert summary_b["best"].tolist() == ["g0", "-", "g1", "-"] and np.allclose(summary_b["best_frac"], [1.0, 0, 0.75, 0])
    assert long_b[["query", "genome"]].values.tolist() == [["q", "g0"], ["q", "g2"], ["q", "g1"]]
    assert long_b.index.tolist() == [0, 1, 2] and len(matrix_b) == 4 and len(summary_b) == 4  # only the long table is cut
    long_k, _, _ = search.frames(names, lens, k, genomes, prof, rows, 0.5)
    assert long_k[["query", "genome"]].values.tolist() == [["q", "g0"], ["q", "g1"], ["q", "g2"], ["q", "g1"], ["q", "g2"]]
    with pytest.raises(ValueError, match="by must be"):
        search.frames(names, lens, k, genomes, prof, rows, by="rows")
    # no query, and no genome
    long, matrix, summary = search.frames([], [], k, genomes, np.zeros((0, 3, 6)), np.zeros((0, 2)))
    assert list(long.columns) == search.LONG_COLUMNS and len(long) == 0 and matrix.shape == (0, 3) and len(summary) == 0
    long, matrix, summary = search.frames(names, lens, k, [], np.zeros((4, 0, 6)), rows)
    assert len(long) == 0 and matrix.shape == (4, 0) and summary["best"].tolist() == ["-"] * 4


def test_pick_genomes():
    assert search.pick_genomes(["a", "b", "c"]) == [0, 1, 2]
    assert search.pick_genomes(["a", "b", "c"], ["c", "a", "c"]) == [0, 2]  # the index's order, once each
    assert search.pick_genomes(["a", "b", "c"], []) == []
    with pytest.raises(KeyError, match="nobody"):
        search.pick_genomes(["a", "b"], ["a", "nobody"])


# ---------------------------------------------------------------------------
# the subcommand, over a stand-in for an open index
# ---------------------------------------------------------------------------
class _Sample:
    def __init__(self, fasta):
        self.fasta = fasta


class _Index:
    """an open index as the subcommand sees it: the names, the samples' sequence files, k, and Index.search itself — which
    builds no table and touches no GPU while no query reaches k bases"""
    k = 5

    def __init__(self, fastas):
        self.genome_names = list(fastas)
        self._samples = {n: _Sample(f) for n, f in fastas.items()}
        self.calls, self.closed = [], False

    def __getitem__(self, name):
        return self._samples[name]

    def _full_table(self):
        raise AssertionError("no table for queries without a k-mer")

    def search(self, queries, genomes=None, min_frac=0.0, by="kmers", batch_bases=None):
        self.calls.append((queries, genomes, min_frac, by, batch_bases))
        return _RealIndex.search(self, queries, genomes, min_frac, by, batch_bases)

    def close(self):
        self.closed = True


def test_cli_search_argument_errors_and_an_empty_query_file(monkeypatch, tmp_path, capsys):
    from panagram_amd import index as pidx
    from panagram_amd.__main__ import main
    fa = tmp_path / "g.fa"
    fa.write_text(">c\nACGTACGT\n")
    idx = _Index({"g0": str(fa), "g1": str(fa)})
    monkeypatch.setattr(pidx, "Index", lambda path, mode=None, device=0: idx)
    index_dir = str(tmp_path)
    empty, short = tmp_path / "empty.fa", tmp_path / "short.fa"
    empty.write_bytes(b"")
    short.write_text(">s1\nACGT\n>s2 x\nAC\nG\n>s1\n\n")

    def fails(argv, *words):
        with pytest.raises(SystemExit) as ei:
            main(argv)
        err = capsys.readouterr().err
        assert ei.value.code == 2 and all(w in err for w in words), err

    fails(["search", str(tmp_path / "nowhere"), str(short)], "search:", "is not an index directory")
    fails(["search", index_dir, str(tmp_path / "missing.fa")], "search: no query file", "missing.fa")
    fails(["search", index_dir, str(short), "--genomes", "g1,nobody"], "search: unknown genome 'nobody'", "g0, g1")
    fails(["search", index_dir, str(short), "--min-frac", "1.5"], "--min-frac")
    fails(["search", index_dir, str(short), "--by", "rows"], "--by")
    fails(["search", index_dir, str(short), "--batch-bases", "0"], "--batch-bases")
    fails(["search", index_dir], "queries.fa")
    assert idx.calls == []
    idx2 = _Index({"g0": str(fa), "g1": str(tmp_path / "gone.fa"), "g2": float("nan")})
    monkeypatch.setattr(pidx, "Index", lambda path, mode=None, device=0: idx2)
    fails(["search", index_dir, str(short)], "search: sample 'g1'", "has no sequence file")
    assert idx2.closed and idx2.calls == []
    monkeypatch.setattr(pidx, "Index", lambda path, mode=None, device=0: (_ for _ in ()).throw(ValueError("no index here")))
    fails(["search", index_dir, str(short)], "search: no index here")
    monkeypatch.setattr(pidx, "Index", lambda path, mode=None, device=0: idx)
    # an empty query file: the header line alone, exit status 0 — on stdout and in all three files
    assert main(["search", index_dir, str(empty)]) == 0
    assert capsys.readouterr().out == "\t".join(search.LONG_COLUMNS) + "\n"
    out, mx, su = tmp_path / "long.tsv", tmp_path / "matrix.tsv", tmp_path / "summary.tsv"
    assert main(["search", index_dir, str(empty), "-o", str(out), "--matrix", str(mx), "--summary", str(su), "--genomes", "g1"]) == 0
    assert out.read_text() == "\t".join(search.LONG_COLUMNS) + "\n" and mx.read_text() == "query\tg1\n"
    assert su.read_text() == "\t".join(search.SUMMARY_COLUMNS) + "\n" and capsys.readouterr().out == ""
    # queries shorter than k: reported with zeros, in file order, duplicate names kept, nothing anchored
    assert main(["search", index_dir, str(short), "-o", str(out), "--matrix", str(mx), "--summary", str(su), "--batch-bases", "3"]) == 0
    assert idx.calls[-1] == (str(short), None, 0.0, "kmers", 3) and idx.closed
    got = pd.read_csv(out, sep="\t")
    assert list(got.columns) == search.LONG_COLUMNS and got["query"].tolist() == ["s1", "s1", "s2", "s2", "s1", "s1"]
    assert got["length"].tolist() == [4, 4, 3, 3, 0, 0] and got["genome"].tolist() == ["g0", "g1"] * 3
    assert not got.drop(columns=["query", "genome", "length"]).to_numpy().any()
    got = pd.read_csv(su, sep="\t")
    assert got["query"].tolist() == ["s1", "s2", "s1"] and got["best"].tolist() == ["-"] * 3 and not got["kmers"].any()
    got = pd.read_csv(mx, sep="\t")
    assert list(got.columns) == ["query", "g0", "g1"] and got["query"].tolist() == ["s1", "s2", "s1"]


def test_index_search_refuses_before_reading():
    idx = _Index({"g0": "x", "g1": "y"})
    with pytest.raises(KeyError, match="nobody"):
        idx.search(b">q\nACGTACGT\n", ["nobody"])
    with pytest.raises(ValueError, match="by must be"):
        idx.search(b">q\nACGTACGT\n", by="rows")
    with pytest.raises(ValueError, match="batch_bases"):
        idx.search(b">q\nACGTACGT\n", batch_bases=0)
    # an empty selection: zeros, and no table
    long, matrix, summary = idx.search(b">q\nACGTACGT\n", [])
    assert len(long) == 0 and matrix.shape == (1, 0) and summary["kmers"].tolist() == [4]


# ---------------------------------------------------------------------------
# the stitch of a window's chunks, and the constants shared with the kernel
# ---------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_profile_stitch_check_program(tmp_path):
    exe = str(tmp_path / "profile_stitch_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tools", "profile_stitch_check.cpp")], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("ok:"), (p.returncode, p.stdout, p.stderr)


def test_chunk_constant_is_the_kernels():
    from panagram_amd import engine
    txt = open(os.path.join(ROOT, "panagram_amd", "csrc", "pg_kernels.h")).read()
    assert int(re.search(r"constexpr uint32_t PROFILE_CHUNK = (\d+);", txt).group(1)) == engine.PROFILE_CHUNK
    assert engine.PROFILE_CHUNK % 256 == 0
    host = open(os.path.join(ROOT, "panagram_amd", "csrc", "pg_profile_host.h")).read()
    assert int(re.search(r"constexpr uint32_t PROFILE_FIELDS = (\d+);", host).group(1)) == len(search.FIELDS) == len(sr.FIELDS)
    assert search.FIELDS == sr.FIELDS
