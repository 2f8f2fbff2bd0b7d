"""GPU: the pan-genome's k-mer statistics end to end on the tiny samples of the index e2e test — `index --kmer_stats`,
`pangenome`, `dist --exact`, Index.kmer_stats() on a filtered table, and the untouched defaults — against the numpy reference
(tests/kmerstats_ref.py) computed from the FASTAs."""
import gzip
import io
import os

import numpy as np
import pandas as pd
import pytest

from oracle import pyoracle as po
from panagram_amd import pangenome
from tests import helpers as H
from tests import kmerstats_ref as KR
from tests import minhash_ref as MR

pytestmark = pytest.mark.gpu

CASE = "n9_k21"


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """the samples on disk, the reference computed from their FASTAs, and the index `index --kmer_stats` wrote"""
    from panagram_amd import __main__ as cli
    tmp = tmp_path_factory.mktemp("pangenome")
    fx = H.load_case(CASE)
    n, k = int(fx["ngenomes"]), int(fx["k"])
    rows, genomes = ["name\tfasta"], []
    for g in range(n):
        fa = tmp / f"g{g}.fa"
        fa.write_bytes(fx[f"fasta_{g}"].tobytes())
        rows.append(f"g{g}\t{fa}")
        genomes.append([seq for _, seq in po.parse_fasta_cpp(fx[f"fasta_{g}"].tobytes())])
    (tmp / "samples.tsv").write_text("\n".join(rows) + "\n")
    keys, M = KR.from_groups(po.build_bitvec_dbs(genomes, k), n)
    ref = KR.stats(keys, M)
    anchors = [f"g{g}" for g in fx["anchors"]]
    assert 0 < len(anchors) < n  # a strict subset: the default table would be a filtered one
    out = tmp / "idx"
    assert cli.main(["index", str(tmp / "samples.tsv"), "-o", str(out), "-k", str(k), "--kmer_stats", "--anchor_genomes"] + anchors) == 0
    return dict(tmp=tmp, out=out, n=n, k=k, ref=ref, names=[f"g{g}" for g in range(n)], anchors=anchors, fx=fx, genomes=genomes)


def test_index_kmer_stats_writes_both_files(case):
    out, n, ref, names = case["out"], case["n"], case["ref"], case["names"]
    text = (out / "kmer_shared.tsv").read_text().splitlines()
    assert text[0].split("\t") == ["name"] + names and [ln.split("\t")[0] for ln in text[1:]] == names
    shared = pd.read_table(out / "kmer_shared.tsv", index_col="name")
    assert list(shared.index) == list(shared.columns) == names
    assert np.array_equal(shared.to_numpy().astype(np.int64), ref["pairs"])
    occ = pd.read_table(out / "kmer_occupancy.tsv")
    assert list(occ.columns) == ["n", "kmers"] and occ["n"].tolist() == list(range(n + 1))
    assert occ["kmers"].tolist() == ref["occupancy"].tolist() and occ["kmers"].sum() == ref["nkeys"]
    assert ref["occupancy"][n] > 0 and ref["occupancy"][1] > 0  # the input stays non-trivial
    assert not [f for f in os.listdir(out) if f.endswith(".tmp")]
    # the anchors' files are there as without the flag
    for a in case["anchors"]:
        assert (out / "anchor" / a / "bitmap.1.gz").exists()


def test_pangenome_subcommand_prints_the_same_table(case, tmp_path, capsys):
    from panagram_amd import __main__ as cli
    ref, names = case["ref"], case["names"]
    _, want = pangenome.frames(ref, names)
    capsys.readouterr()
    assert cli.main(["pangenome", str(case["out"]), "--matrix", str(tmp_path / "m.tsv"), "--occupancy", str(tmp_path / "o.tsv")]) == 0
    printed = capsys.readouterr().out
    lines = [ln for ln in printed.splitlines() if ln.count("\t") == 4]
    assert lines[0].split("\t") == ["name", "kmers", "private", "core", "shell"]
    got = pd.read_table(io.StringIO("\n".join(lines)), index_col="name")
    assert list(got.index) == names and np.array_equal(got.to_numpy().astype(np.int64), want.to_numpy())
    assert (tmp_path / "m.tsv").read_bytes() == (case["out"] / "kmer_shared.tsv").read_bytes()
    assert (tmp_path / "o.tsv").read_bytes() == (case["out"] / "kmer_occupancy.tsv").read_bytes()


def test_dist_exact_writes_exact_distances_in_the_files_layout(case):
    from panagram_amd import __main__ as cli
    out, n, k, ref, names = case["out"], case["n"], case["k"], case["ref"], case["names"]
    assert cli.main(["dist", str(out)]) == 0
    default = (out / "genome_dist.tsv").read_bytes()
    assert cli.main(["dist", str(out), "--exact"]) == 0
    text = (out / "genome_dist.tsv").read_text()
    assert text.splitlines() == [ln.rstrip("\n") for ln in pangenome.genome_dist_lines(names, ref["pairs"], k)]
    got = pd.read_table(out / "genome_dist.tsv", names=["a", "b", "dist", "p", "frac"])
    old = pd.read_table(io.BytesIO(default), names=["a", "b", "dist", "p", "frac"])
    assert len(got) == n * (n - 1) // 2 and got[["a", "b"]].equals(old[["a", "b"]])
    assert got.dtypes["dist"] == old.dtypes["dist"] == np.float64
    j, d = pangenome.exact_distances(ref["pairs"], k)
    assert got["dist"].tolist() == [float(f"{x:.6g}") for x in d] and (got["p"] == 0).all()
    c = ref["pairs"]
    assert got["frac"].tolist() == [f"{c[a, b]}/{c[a, a] + c[b, b] - c[a, b]}" for a in range(n) for b in range(a + 1, n)]
    assert 0 < d.min() and d.max() < 1
    # and the default writes again what it wrote before
    assert cli.main(["dist", str(out)]) == 0
    assert (out / "genome_dist.tsv").read_bytes() == default


def test_a_cached_filtered_table_refuses(case):
    from panagram_amd import index as pidx
    idx = pidx.Index(str(case["tmp"] / "samples.tsv"), prefix=str(case["tmp"] / "filtered"), k=case["k"], anchor_genomes=case["anchors"],
                     filtered_table=True)
    try:
        idx.build_table()
        assert idx._table_scope == frozenset(case["anchors"])
        with pytest.raises(RuntimeError, match="the cached table was built for the anchors .* only"):
            idx.kmer_stats()
        with pytest.raises(RuntimeError, match="only"):
            idx.write_kmer_stats()
        idx.close()
        # no table cached: one of all samples' k-mers is built, whatever the anchors, and cached as such
        shared, genomes = idx.kmer_stats()
        assert idx._table_scope == "all" and idx._table is not None
        assert np.array_equal(shared.to_numpy(), case["ref"]["pairs"])
        assert genomes["private"].tolist() == case["ref"]["private"].tolist()
    finally:
        idx.close()


def test_without_the_flag_nothing_changes(case):
    from panagram_amd import index as pidx
    from panagram_amd.index import read_fasta
    tmp, names = case["tmp"], case["names"]
    out = tmp / "plain"
    idx = pidx.Index(str(tmp / "samples.tsv"), prefix=str(out), k=case["k"], anchor_genomes=case["anchors"], genome_dist=True)
    assert not idx.kmer_stats
    idx.run()
    assert not (out / "kmer_shared.tsv").exists() and not (out / "kmer_occupancy.tsv").exists()
    recs = [[seq for _, seq in read_fasta(str(tmp / f"{g}.fa"))] for g in names]
    assert (out / "genome_dist.tsv").read_text() == MR.genome_dist_text(names, [MR.sketch(r) for r in recs], [MR.acgt_bases(r) for r in recs])
    # the rows of the anchors do not depend on the flag
    for a in case["anchors"]:
        assert (out / "anchor" / a / "bitsum.bins.tsv").read_bytes() == (case["out"] / "anchor" / a / "bitsum.bins.tsv").read_bytes(), a
        assert gzip.open(out / "anchor" / a / "bitmap.1.gz").read() == gzip.open(case["out"] / "anchor" / a / "bitmap.1.gz").read(), a
