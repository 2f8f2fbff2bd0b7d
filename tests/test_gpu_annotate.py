"""GPU: `annotate` (Genome.run_annotate) on indexes written by Index.run(): per-gene occupancy from bitmap.1.gz inflated on
the GPU against the oracle's rows, bitsum.genes.tsv and chrs.tsv against what the anchoring run wrote, and `index --annotate`
against `index` followed by `annotate` — one rank, two contig-sharded ranks, host-level and GPU-compressed bitmaps."""
import gzip
import os
import shutil

import numpy as np
import pandas as pd
import pytest

from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

K, N = 21, 3
NAMES = ["chrB", "chrA", "chrC"]
GENES = [("chrA", 100, 900), ("chrA", 850, 2000), ("chrA", 850, 2000), ("chrB", 1, 19000), ("chrB", 500, 400),
         ("chrB", 19000, 20001), ("chrZ", 10, 20), ("chrC", 0, 980)]


@pytest.fixture(scope="module")
def pangenome():
    gen = po.synth_genomes(N, [20000, 8000, 1000], 0.02, 5)
    genomes = [[po.codes_to_ascii(c) for c in g] for g in gen]
    dbs = po.build_bitvec_dbs(genomes, K)
    rows = {c: po.anchor_contig(dbs, genomes[0][i], K, N)[0] for i, c in enumerate(NAMES)}
    return genomes, rows


def write_inputs(tmp_path, genomes, with_gff=True):
    gff = tmp_path / "g0.gff"
    with open(gff, "w") as f:
        f.write("##gff-version 3\n")
        for i, (c, s, e) in enumerate(GENES):
            f.write(f"{c}\tsrc\tgene\t{s}\t{e}\t.\t+\t.\tID=g{i};Name=n{i}\n")
            f.write(f"{c}\tsrc\tmRNA\t{s}\t{e}\t.\t+\t.\tID=t{i};Parent=g{i}\n")
            f.write(f"{c}\tsrc\texon\t{s}\t{e}\t.\t+\t.\tParent=t{i}\n")
            f.write(f"{c}\tsrc\tCDS\t{s}\t{e}\t.\t+\t0\tParent=t{i}\n")
    rows = ["name\tfasta\tgff"]
    for g in range(N):
        fa = tmp_path / f"g{g}.fa"
        fa.write_bytes(po.fasta_text(NAMES, genomes[g]))
        rows.append(f"g{g}\t{fa}\t" + (str(gff) if g == 0 and with_gff else ""))
    (tmp_path / "samples.tsv").write_text("\n".join(rows) + "\n")
    return str(tmp_path / "samples.tsv"), str(gff)


def track(d, typ):
    p = os.path.join(d, "anchor", "g0", f"{typ}.bed.gz")
    return gzip.decompress(open(p, "rb").read()), open(p + ".csi", "rb").read()


def test_annotate_matches_oracle_and_anchoring_run(tmp_path, pangenome):
    from panagram_amd import index as pidx
    from panagram_amd.__main__ import main
    genomes, orows = pangenome
    samples, gff = write_inputs(tmp_path, genomes)
    out = str(tmp_path / "idx")
    pidx.Index(samples, prefix=out, k=K, anchor_genomes=["g0"]).run()
    gdir = os.path.join(out, "anchor", "g0")
    genes_tsv = open(os.path.join(gdir, "bitsum.genes.tsv"), "rb").read()
    chrs_tsv = open(os.path.join(gdir, "chrs.tsv"), "rb").read()
    assert not os.path.exists(os.path.join(gdir, "gene.bed.gz"))  # (the default tree is unchanged)
    assert main(["annotate", out, "g0", gff]) == 0
    assert open(os.path.join(gdir, "bitsum.genes.tsv"), "rb").read() == genes_tsv
    assert open(os.path.join(gdir, "chrs.tsv"), "rb").read() == chrs_tsv
    idx = pidx.Index(out, mode="r")
    got = idx.query_genes("g0")
    assert list(got.columns) == ["chr", "start", "end", "name", 1, N]
    want = []
    for i, (c, s, e) in enumerate(GENES):
        h = np.zeros(N + 1, np.int64)
        if c in orows and e > s and s >= 0 and e <= len(orows[c]):
            h = po.window_stats(orows[c], N, [s], [e])[0][0]
        want.append((c, s, e, f"n{i}", int(h[1]), int(h[N])))
    want = sorted(want, key=lambda r: (r[0], r[1]))
    assert [tuple(r) for r in got.itertuples(index=False, name=None)] == want
    assert np.any(got[N] > 0) and np.any(got[1] > 0)
    sub = idx.query_genes("g0", "chrA", 950, 1000)
    assert sorted(sub["name"]) == ["n1", "n2"]
    anno = idx.query_anno("g0", "chrA", 0, 10 ** 6)
    assert set(anno["type"]) == {"mRNA", "exon", "CDS"} and set(anno["name"]) == {"n0", "n1", "n2"}
    assert list(anno.columns) == ["chr", "start", "end", "type", "name", "type_id"]
    assert (anno.loc[anno["type"] == "exon", "type_id"] == 0).all()
    assert open(os.path.join(gdir, "anno_types.txt")).read() == "CDS\nexon\nmRNA\n"
    idx.close()


def test_annotate_unannotated_index_changes_only_gene_count(tmp_path, pangenome):
    from panagram_amd import index as pidx
    genomes, _ = pangenome
    samples, gff = write_inputs(tmp_path, genomes, with_gff=False)
    out = str(tmp_path / "idx")
    pidx.Index(samples, prefix=out, k=K, anchor_genomes=["g0"]).run()
    gdir = os.path.join(out, "anchor", "g0")
    before = pd.read_table(os.path.join(gdir, "chrs.tsv"))
    idx = pidx.Index(out, mode="r")
    idx["g0"].run_annotate(gff, nogene=True)
    assert os.path.exists(os.path.join(gdir, "anno.bed.gz.csi")) and not os.path.exists(os.path.join(gdir, "gene.bed.gz"))
    idx["g0"].run_annotate(gff)
    idx.close()
    after = pd.read_table(os.path.join(gdir, "chrs.tsv"))
    assert after.drop(columns="gene_count").equals(before.drop(columns="gene_count"))
    assert after.set_index("name")["gene_count"].to_dict() == {"chrB": 3, "chrA": 3, "chrC": 1}


@pytest.mark.parametrize("mode", ["one_rank", "contig_sharded", "host_level"])
def test_index_annotate_equals_index_then_annotate(tmp_path, pangenome, mode):
    from panagram_amd import index as pidx
    genomes, _ = pangenome
    samples, gff = write_inputs(tmp_path, genomes)
    ref = str(tmp_path / "ref")
    pidx.Index(samples, prefix=ref, k=K, anchor_genomes=["g0"]).run()
    pidx.Index(ref, mode="r")["g0"].run_annotate()
    out = str(tmp_path / "ann")
    if mode == "contig_sharded":
        for rank in range(2):
            pidx.Index(samples, prefix=out, k=K, anchor_genomes=["g0"], rank=rank, world=2, annotate=True).run()
    else:
        idx = pidx.Index(samples, prefix=out, k=K, anchor_genomes=["g0"], annotate=True)
        if mode == "host_level":
            idx.bgzf_level = 6  # bitmap.1.gz compressed by host zlib instead of k_row_deflate
        idx.run()
    for typ in ("gene", "anno"):
        assert track(out, typ) == track(ref, typ), typ
    for f in ("anno_types.txt", "bitsum.genes.tsv", "chrs.tsv"):
        assert open(os.path.join(out, "anchor", "g0", f), "rb").read() == open(os.path.join(ref, "anchor", "g0", f), "rb").read(), f
