"""GPU: Index.copies, Genome.gene_copies and the `copies` subcommand on an index written by Index.run() — three small genomes with
genes planted in known numbers — against ``copies.frames`` of the numpy model's arrays (tests/copies_ref.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle as po
from panagram_amd import copies as cp
from tests import copies_ref as cr

pytestmark = pytest.mark.gpu

K = 21
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["g0", "g1", "g2"]
CHROMS = ["chr1", "chr2"]
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def rand(rng, n):
    return bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)])


def revcomp(s):
    return s.translate(_COMP)[::-1]


def _genomes():
    """per genome its two chromosomes, and the three genes: A 1 / 3 / 0 copies, B 1 / 1 (with one substitution) / 0, C 1 / 0 / 0"""
    rng = np.random.default_rng(41)
    a, b, c = rand(rng, 1500), rand(rng, 900), rand(rng, 400)
    f = [rand(rng, 700) for _ in range(8)]
    b_sub = bytearray(b)
    b_sub[300] = b"ACGT"[(b"ACGT".index(b_sub[300]) + 1) % 4]
    g0 = [f[0][:613] + a + f[1] + b + f[2], f[3][:77] + c + f[4]]
    g1 = [f[5] + a + f[6] + revcomp(a) + f[0] + a.lower(), bytes(b_sub) + f[7]]
    g2 = [rand(rng, 3000) + b"NNNNN" + rand(rng, 500).lower(), rand(rng, 1000)]
    genes = [("chr1", 613, 613 + 1500), ("chr1", 613 + 1500 + 700, 613 + 1500 + 700 + 900), ("chr2", 77, 77 + 400),
             ("chrZ", 10, 500), ("chr1", 900, 880), ("chr2", 1100, 5000)]
    return [g0, g1, g2], dict(a=a, b=b, c=c), genes


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    from panagram_amd import index as pidx
    tmp = tmp_path_factory.mktemp("copies")
    genomes, _, genes = _genomes()
    gff = tmp / "g0.gff"
    with open(gff, "w") as fh:
        fh.write("##gff-version 3\n")
        for i, (c, s, e) in enumerate(genes):
            fh.write(f"{c}\tsrc\tgene\t{s}\t{e}\t.\t+\t.\tID=g{i}\n")
            fh.write(f"{c}\tsrc\texon\t{s}\t{e}\t.\t+\t.\tParent=g{i}\n")
    lines = ["name\tfasta\tgff"]
    for i, contigs in enumerate(genomes):
        fa = tmp / f"g{i}.fa"
        fa.write_bytes(po.fasta_text(CHROMS, contigs))
        lines.append(f"g{i}\t{fa}\t" + (str(gff) if i == 0 else ""))
    (tmp / "samples.tsv").write_text("\n".join(lines) + "\n")
    out = str(tmp / "idx")
    pidx.Index(str(tmp / "samples.tsv"), prefix=out, k=K, anchor_genomes=["g0"], lowres_step=100).run()
    return out


def targets():
    """[(name, sequence)], in file order: a duplicate name, a target shorter than k, an empty one, one with N"""
    genomes, g, _ = _genomes()
    a = g["a"]
    return [("geneA", a), ("geneB", g["b"]), ("geneC", g["c"]), ("geneA_rc", revcomp(a)), ("short", a[:K - 1]), ("geneA", a[200:700].lower()),
            ("empty", b""), ("withN", a[:300] + b"N" + a[301:600]), ("exact", a[40:40 + K])]


def fasta(width=60):
    out = []
    for i, (name, seq) in enumerate(targets()):
        out.append(b">" + name.encode() + (b" a description" if i == 1 else b"") + b"\n")
        out += [seq[j:j + width] + b"\n" for j in range(0, len(seq), width)]
    return b"".join(out)


def reference(named, cols=(0, 1, 2), k=K):
    genomes = _genomes()[0]
    seqs = [s for _, s in named]
    hist, valid, track = cr.profile(seqs, [genomes[c] for c in cols], k)
    frames = cp.frames([n for n, _ in named], [len(s) for s in seqs], k, [NAMES[c] for c in cols], hist, valid)
    return frames, track


def _same(got, want, tag):
    for g, w, what in zip(got, want, ("long", "matrix", "summary")):
        assert g.to_csv(sep="\t") == w.to_csv(sep="\t"), (tag, what)


def test_copies_equals_the_model(built, monkeypatch):
    from panagram_amd import index as pidx
    want, wtrack = reference(targets())
    idx = pidx.Index(built, mode="r")
    try:
        got = idx.copies(fasta())
        _same(got, want, "fasta")
        long, matrix, summary = got
        assert matrix.index.tolist() == [n for n, _ in targets()]
        assert matrix["g0"].tolist() == [1, 1, 1, 1, 0, 1, 0, 1, 1] and matrix["g1"].tolist() == [3, 1, 0, 3, 0, 3, 0, 3, 3]
        assert not matrix["g2"].any()
        b1 = long[(long["target"] == "geneB") & (long["genome"] == "g1")].iloc[0]
        assert b1["present"] == b1["valid"] - K and b1["copies"] == 1  # (the substitution takes the k windows over it)
        assert summary.to_numpy().tolist() == [["g0", 9, 2, 7, 0, 0, 0], ["g1", 9, 3, 1, 0, 5, 0], ["g2", 9, 9, 0, 0, 0, 0]]
        # a list of (name, sequence); with the track; a selection in another order and another k
        assert not idx._seqsets  # (what the call loaded it dropped again)
        again = idx.copies(targets(), track=True)
        _same(again[:3], want, "pairs")
        assert np.array_equal(again[3], wtrack)
        sub = idx.copies(targets(), ["g2", "g1"], k=15, track=True)
        wsub, wt = reference(targets(), (1, 2), 15)
        _same(sub[:3], wsub, "selection")
        assert np.array_equal(sub[3], wt) and sub[1].columns.tolist() == ["g1", "g2"]
        # batches of two planes and of one: the second batch counts into planes that were cleared
        for per in (2, 1):
            monkeypatch.setattr(cp, "planes_for", lambda *args, **kw: per)
            small = idx.copies(targets(), track=True)
            _same(small[:3], want, f"{per} planes")
            assert np.array_equal(small[3], wtrack)
        monkeypatch.undo()
        held = idx.seqset_for("g1")  # a sequence set that was loaded before stays
        idx.copies(targets()[:1], ["g1"])
        assert idx._seqsets.get("g1") is held
        with pytest.raises(KeyError, match="nobody"):
            idx.copies(targets(), ["nobody"])
        with pytest.raises(ValueError, match="k=33"):
            idx.copies(targets(), k=33)
        assert len(idx.copies(b"")[0]) == 0
    finally:
        idx.close()


def test_gene_copies_on_a_small_gff(built):
    from panagram_amd import index as pidx
    genomes, _, genes = _genomes()
    chrom = dict(zip(CHROMS, genomes[0]))
    order = sorted(range(len(genes)), key=lambda i: (genes[i][0], genes[i][1]))  # (load_genes sorts by chromosome and start)
    named = [(f"{genes[i][0]}:{genes[i][1]}-{genes[i][2]}", chrom.get(genes[i][0], b"")[genes[i][1]:max(genes[i][1], genes[i][2])]) for i in order]
    want, wtrack = reference(named)
    idx = pidx.Index(built, mode="r")
    try:
        got = idx["g0"].gene_copies(track=True)
        _same(got[:3], want, "genes")
        assert np.array_equal(got[3], wtrack)
        m = got[1]
        assert m.loc["chr1:613-2113"].tolist() == [1, 3, 0] and m.loc["chr2:77-477"].tolist() == [1, 0, 0]
        assert m.loc["chrZ:10-500"].tolist() == [0, 0, 0] and m.loc["chr1:900-880"].tolist() == [0, 0, 0]
        with pytest.raises(ValueError, match="GFF"):
            idx["g1"].gene_copies()
    finally:
        idx.close()


def test_copies_subcommand_in_a_child_process(built, tmp_path):
    (want_long, want_matrix, want_summary), wtrack = reference(targets())
    tfa = tmp_path / "targets.fa"
    tfa.write_bytes(fasta(70))
    out, mx, su, tr = (tmp_path / n for n in ("long.tsv", "matrix.tsv", "summary.tsv", "track.tsv"))
    p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "panagram_amd", "copies", built, str(tfa), "-o", str(out),
                        "--matrix", str(mx), "--summary", str(su), "--track", str(tr)], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    assert out.read_text() == cp.long_text(want_long).to_csv(sep="\t", index=False)
    assert mx.read_text() == cp.matrix_text(want_matrix).to_csv(sep="\t", index_label="target")
    assert su.read_text() == want_summary.to_csv(sep="\t", index=False)
    names, lens = [n for n, _ in targets()], [len(s) for _, s in targets()]
    assert tr.read_text().split("\n")[:-1] == [cp.TRACK_HEADER] + list(cp.track_lines(names, lens, K, NAMES, wtrack))
    # an unknown genome name: an argparse error that names it
    p = subprocess.run([sys.executable, "-m", "panagram_amd", "copies", built, str(tfa), "--genomes", "g1,nobody"], cwd=ROOT,
                       capture_output=True, text=True)
    assert p.returncode == 2 and "nobody" in p.stderr
