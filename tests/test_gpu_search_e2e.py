"""GPU: Index.search and the `search` subcommand on an index written by Index.run() — the planted-variant genomes of
tests/gaps_ref.py and a third, unrelated one, as tests/test_gpu_gaps_e2e.py builds it — against the numpy model of the presence
profile (tests/search_ref.py) applied to the rows the oracle gives for the QUERY sequences: queries that are not in the index
are anchored against the k-mers of every sample."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from oracle import pyoracle as po
from panagram_amd import search
from tests import gaps_ref as gr
from tests import search_ref as sr

pytestmark = pytest.mark.gpu

K = gr.PLANTED_K
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["g0", "g1", "g2"]
SEG = (400, 1100)  # of g0: spans the substitution at 500 and the two at 900 and 907


def _genomes():
    a, b = gr.planted_genomes()
    other = np.random.default_rng(99).integers(0, 4, gr.PLANTED_LEN, dtype=np.uint8)
    return [po.codes_to_ascii(c) for c in (a, b, other)]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    from panagram_amd import index as pidx
    tmp = tmp_path_factory.mktemp("search")
    lines = ["name\tfasta"]
    for i, seq in enumerate(_genomes()):
        fa = tmp / f"g{i}.fa"
        fa.write_bytes(po.fasta_text(["chr1"], [seq]))
        lines.append(f"g{i}\t{fa}")
    (tmp / "samples.tsv").write_text("\n".join(lines) + "\n")
    out = str(tmp / "idx")
    pidx.Index(str(tmp / "samples.tsv"), prefix=out, k=K, anchor_genomes=["g0"], lowres_step=100).run()
    return out


def _revcomp(seq: bytes) -> bytes:
    return seq.translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))[::-1]


def queries():
    """[(name, sequence)], in file order: a duplicate name among them"""
    g0 = _genomes()[0]
    seg = g0[SEG[0]:SEG[1]]
    with_n = seg[:300] + b"N" * 7 + seg[307:]
    rnd = po.codes_to_ascii(np.random.default_rng(5).integers(0, 4, 500, dtype=np.uint8))
    return [("seg", seg), ("seg_rc", _revcomp(seg)), ("seg_lower", seg.lower()), ("seg_n", with_n), ("random", rnd),
            ("short", g0[50:50 + K - 1]), ("exact", g0[1500:1500 + K]), ("seg", g0[1300:2100]), ("empty", b"")]


def fasta(width=60):
    """the queries as multi-line records, the header of one with a description"""
    out = []
    for i, (name, seq) in enumerate(queries()):
        out.append(b">" + name.encode() + (b" a description" if i == 1 else b"") + b"\n")
        out += [seq[j:j + width] + b"\n" for j in range(0, len(seq), width)]
    return b"".join(out)


def reference(cols=None):
    """(profile [queries, 3, 6], rows [queries, 2]) by the model on the oracle's rows of every query"""
    dbs = po.build_bitvec_dbs([[g] for g in _genomes()], K)
    prof, allnone = [], []
    for _, seq in queries():
        masks = po.counters_for_read(dbs[0], seq, K)  # (one mask per k-mer: bit g = sample g holds it; none for a short query)
        bits = ((masks[:, None] >> np.arange(3, dtype=np.uint32)[None, :]) & 1).astype(np.uint8)
        p, an = sr.ref_window(bits, K, cols)
        prof.append(p)
        allnone.append(an)
    return np.stack(prof), np.array(allnone, np.int64)


def _same(got, want, tag):
    assert list(got.columns) == list(want.columns) and len(got) == len(want), (tag, list(got.columns), len(got), len(want))
    for col in want.columns:
        a, b = got[col].to_numpy(), want[col].to_numpy()
        if b.dtype.kind == "f":
            assert np.allclose(a.astype(float), b, rtol=0, atol=1e-12), (tag, col)
        else:
            assert a.tolist() == b.tolist(), (tag, col, a.tolist()[:12], b.tolist()[:12])


def test_search_equals_the_model_on_the_oracles_rows(built):
    from panagram_amd import index as pidx
    names = [n for n, _ in queries()]
    lens = [len(s) for _, s in queries()]
    prof, allnone = reference()
    idx = pidx.Index(built, mode="r")
    try:
        got = idx.search(fasta())
        want = search.frames(names, lens, K, NAMES, prof, allnone)
        for g, w, what in zip(got, want, ("long", "matrix", "summary")):
            _same(g.reset_index() if what == "matrix" else g, w.reset_index() if what == "matrix" else w, what)
        long, matrix, summary = got
        # what the queries are there for
        q = {(r.query, r.genome, i // 3): r for i, r in enumerate(long.itertuples())}
        n = SEG[1] - SEG[0] - K + 1
        seg0, seg1, seg2 = q["seg", "g0", 0], q["seg", "g1", 0], q["seg", "g2", 0]
        assert (seg0.hits, seg0.runs, seg0.longest, seg0.first, seg0.end, seg0.covered) == (n, 1, n, 0, n, n + K - 1)
        assert seg0.frac == 1.0 and seg0.cov_frac == 1.0
        assert seg1.hits == n - 21 - 28 and seg1.runs == 3 and seg1.covered == n + K - 1 - 1 - 8  # one base, and bases 900..907
        assert seg1.cov_frac > 0.98 > seg1.frac and seg2.hits == 0 and seg2.covered == 0
        for g in range(3):  # the reverse complement: the same k-mers in reverse order
            fwd, rev = long.iloc[g], long.iloc[3 + g]
            assert rev.query == "seg_rc" and [rev.hits, rev.runs, rev.longest, rev.covered] == [fwd.hits, fwd.runs, fwd.longest, fwd.covered]
            assert (rev["first"], rev.end) == ((n - fwd.end, n - fwd["first"]) if fwd.hits else (0, 0))
            low = long.iloc[6 + g]
            assert low.query == "seg_lower" and low.iloc[4:].tolist() == fwd.iloc[4:].tolist()
        with_n = q["seg_n", "g0", 3]
        assert with_n.hits == n - (7 + K - 1) and with_n.runs == 2 and with_n.covered == SEG[1] - SEG[0] - 7
        assert not long[long["query"] == "random"][["hits", "covered"]].to_numpy().any()
        assert long[long["query"] == "short"]["kmers"].tolist() == [0, 0, 0] and q["exact", "g0", 6].hits == 1 and q["exact", "g0", 6].covered == K
        assert summary["query"].tolist() == names and names.count("seg") == 2
        assert summary["best"].tolist() == ["g0", "g0", "g0", "g0", "-", "-", "g0", "g0", "-"]
        assert summary.loc[0, ["all", "none"]].tolist() == [0, 0] and summary.loc[4, "none"] == 500 - K + 1
        # every record a batch of its own, and a few per batch: the same frames
        for batch_bases in (1, 1500):
            again = idx.search(fasta(), batch_bases=batch_bases)
            assert all(a.equals(b) for a, b in zip(again, got)), batch_bases
        # a path, gzipped; a list of (name, sequence); a selection, by bases, with a floor
        assert all(a.equals(b) for a, b in zip(idx.search(queries()), got))
        sub = idx.search(queries(), ["g2", "g1"], 0.5, "bases")
        psub, asub = reference([1, 2])
        want = search.frames(names, lens, K, ["g1", "g2"], psub[:, [1, 2]], asub, 0.5, "bases")
        for g, w, what in zip(sub, want, ("long", "matrix", "summary")):
            _same(g.reset_index() if what == "matrix" else g, w.reset_index() if what == "matrix" else w, "selection " + what)
        assert set(sub[0]["genome"]) == {"g1"} and len(sub[0]) == 6 and sub[2].loc[0, "none"] == 21 + 28
        with pytest.raises(KeyError, match="nobody"):
            idx.search(queries(), ["nobody"])
    finally:
        idx.close()


def test_search_subcommand_in_a_child_process(built, tmp_path):
    names = [n for n, _ in queries()]
    lens = [len(s) for _, s in queries()]
    prof, allnone = reference()
    want = search.frames(names, lens, K, NAMES, prof, allnone, 0.4)
    import gzip
    qfa = tmp_path / "queries.fa.gz"
    with gzip.open(qfa, "wb") as f:
        f.write(fasta(70))
    out, mx, su = tmp_path / "long.tsv", tmp_path / "matrix.tsv", tmp_path / "summary.tsv"
    p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "panagram_amd", "search", built, str(qfa), "-o", str(out),
                        "--matrix", str(mx), "--summary", str(su), "--min-frac", "0.4", "--batch-bases", "2000"], cwd=ROOT,
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    got = pd.read_csv(out, sep="\t")
    _same(got, want[0], "-o")
    assert len(got) == 12 and got["frac"].min() >= 0.4
    _same(pd.read_csv(mx, sep="\t"), want[1].reset_index(), "--matrix")
    got = pd.read_csv(su, sep="\t")
    _same(got, want[2], "--summary")
    assert got["query"].tolist() == names
    # an empty query file: the header line alone, exit status 0
    empty = tmp_path / "empty.fa"
    empty.write_bytes(b"")
    p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "panagram_amd", "search", built, str(empty)], cwd=ROOT,
                       capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout == "\t".join(search.LONG_COLUMNS) + "\n", (p.returncode, p.stdout, p.stderr[-2000:])
    # an unknown genome name: an argparse error that names it
    p = subprocess.run([sys.executable, "-m", "panagram_amd", "search", built, str(qfa), "--genomes", "g1,nobody"], cwd=ROOT,
                       capture_output=True, text=True)
    assert p.returncode == 2 and "nobody" in p.stderr
