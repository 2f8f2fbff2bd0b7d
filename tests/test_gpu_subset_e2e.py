"""GPU: `subset` end to end on the golden fixtures: ``Index.run()`` over all samples, then ``Index.subset``, gives the tree a
from-scratch ``Index.run()`` over a samples table of the kept samples in kept order gives — under the rule of
tests/test_gpu_add_e2e.py's ``_same_index_payload`` (decompressed bitmaps and every table byte for byte) — and its queries
return the selected bits of the golden payload."""
import os
import shutil

import numpy as np
import pandas as pd
import pytest

from oracle import pyoracle as po
from tests import helpers as H
from tests.test_gpu_add_e2e import _gff_for, _same_index_payload, _tables, _tree_bytes

pytestmark = pytest.mark.gpu


def _kept_table(tmp_path, allp, kept, anchors=None, tag="kept"):
    """a samples table of the kept samples in kept order, as a user would write it for `index`"""
    t = pd.read_table(allp).set_index("name").loc[list(kept)].reset_index()
    if anchors is not None:
        t["anchor"] = t["name"].isin(list(anchors))
    p = tmp_path / f"samples_{tag}.tsv"
    t.to_csv(p, sep="\t", index=False)
    return str(p)


def _run(table, prefix, k, **kw):
    from panagram_amd import index as pidx
    pidx.Index(table, prefix=str(prefix), k=k, **kw).run()
    return prefix


def _subset(src, out, **kw):
    from panagram_amd import index as pidx
    idx = pidx.Index(str(src), mode="r")
    try:
        return idx.subset(str(out), **kw)
    finally:
        idx.close()


def _lines(fx, kept, anchors=None):
    """what subset prints: one line per anchor of the source, in the source's order"""
    n = int(fx["ngenomes"])
    written = [g for g in kept if g in {int(a) for a in fx["anchors"]} and (anchors is None or g in anchors)]
    return [f"rewrote anchor g{g}: {n} -> {len(kept)} samples" if g in written else f"dropped anchor g{g}"
            for g in sorted(int(a) for a in fx["anchors"])]


def _check_queries(out, fx, kept):
    """the read side of the new tree: query == the selected bits of the golden payload of all samples"""
    from panagram_amd import index as pidx
    n, k = int(fx["ngenomes"]), int(fx["k"])
    ridx = pidx.Index(str(out), mode="r")
    assert list(ridx.genome_names) == [f"g{i}" for i in kept]
    assert list(ridx.samples["id"]) == list(range(len(kept)))
    g = next(int(a) for a in fx["anchors"] if int(a) in kept)
    rows = np.frombuffer(fx[f"a{g}_bitmap1"].tobytes(), np.uint8).reshape(-1, (n + 7) // 8)
    bits = np.unpackbits(rows, axis=1, bitorder="little")[:, kept]
    off = 0
    for nm, seq in po.parse_fasta_cpp(fx[f"fasta_{g}"].tobytes()):
        nk = len(seq) - k + 1
        df = ridx.query_bitmap(f"g{g}", nm, 100, min(nk, 700))
        assert list(df.columns) == [f"g{i}" for i in kept]
        assert np.array_equal(df.to_numpy(), bits[off + 100: off + min(nk, 700)])
        assert np.array_equal(ridx.query_bitmap(f"g{g}", nm, 0, nk, 100).to_numpy(), bits[off: off + nk: 100])
        off += nk


# (case, the kept samples in kept order, how they are asked for)
CASES = [("n2_k21", [0], "keep"),                                         # one sample of two
         ("n9_k21", [0, 1, 2, 3, 4, 5, 6, 7], "drop"),                    # 9 -> 8, the last sample (an anchor) dropped
         ("n9_k21", [0, 1, 2, 3, 5, 6, 7, 8], "drop"),                    # an anchor in the middle dropped
         ("n65_k21", [g for g in range(65) if g != 32], "drop"),          # 65 -> 64: nine bytes -> eight
         ("n40_k31", [33, 2, 39, 17, 0, 8, 31, 32], "keep"),              # 8 of 40 in shuffled order
         ("n65_k21", [64] + list(range(1, 65, 2)), "keep")]               # 33 of 65, the last one first


@pytest.mark.parametrize("name, kept, how", CASES, ids=[f"{c}_{h}_{len(kp)}_case{i}" for i, (c, kp, h) in enumerate(CASES)])
def test_subset_gives_the_fresh_tree(name, kept, how, tmp_path):
    fx = H.load_case(name)
    n, k = int(fx["ngenomes"]), int(fx["k"])
    _, allp = _tables(tmp_path, fx, [])
    src = _run(allp, tmp_path / "idx", k)
    before = _tree_bytes(src)
    out = tmp_path / "sub"
    if how == "keep":
        lines = _subset(src, out, keep=[f"g{g}" for g in kept])
    else:
        lines = _subset(src, out, drop=",".join(f"g{g}" for g in range(n) if g not in kept))
    assert lines == _lines(fx, kept)
    assert _tree_bytes(src) == before  # the source is never touched
    for g in (int(a) for a in fx["anchors"]):
        assert (out / "anchor" / f"g{g}").is_dir() == (g in kept)
    _check_queries(out, fx, kept)
    fresh = _run(_kept_table(tmp_path, allp, [f"g{g}" for g in kept]), tmp_path / "fresh", k)
    _same_index_payload(str(fresh), str(out))


def test_anchors_narrows_the_anchors_written(tmp_path):
    fx = H.load_case("n9_k21")
    k = int(fx["k"])
    _, allp = _tables(tmp_path, fx, [])
    src = _run(allp, tmp_path / "idx", k)
    kept = list(range(8))
    out = tmp_path / "sub"
    assert _subset(src, out, drop="g8", anchors="g4") == _lines(fx, kept, anchors=[4])
    assert sorted(os.listdir(out / "anchor")) == ["g4"]
    fresh = _run(_kept_table(tmp_path, allp, [f"g{g}" for g in kept], anchors=["g4"]), tmp_path / "fresh", k)
    _same_index_payload(str(fresh), str(out))


def test_subset_of_a_subset_equals_the_direct_subset(tmp_path):
    fx = H.load_case("n9_k21")
    _, allp = _tables(tmp_path, fx, [])
    src = _run(allp, tmp_path / "idx", int(fx["k"]))
    _subset(src, tmp_path / "s1", drop="g8,g1")
    assert _subset(tmp_path / "s1", tmp_path / "s2", keep="g5,g0,g4,g2") == ["rewrote anchor g0: 7 -> 4 samples", "rewrote anchor g4: 7 -> 4 samples"]
    _subset(src, tmp_path / "direct", keep="g5,g0,g4,g2")
    _same_index_payload(str(tmp_path / "direct"), str(tmp_path / "s2"))
    _check_queries(tmp_path / "s2", fx, [5, 0, 4, 2])


def test_add_then_subset_gives_back_the_original_tree(tmp_path):
    from panagram_amd import index as pidx
    fx = H.load_case("n9_k21")
    (old_tsv, new_tsv), _ = _tables(tmp_path, fx, [7])
    idx_dir = _run(old_tsv, tmp_path / "idx", int(fx["k"]))
    shutil.copytree(idx_dir, tmp_path / "original")
    idx = pidx.Index(str(idx_dir), mode="w")
    idx.add(new_tsv)
    idx.close()
    _subset(idx_dir, tmp_path / "back", drop="g7,g8")
    _same_index_payload(str(tmp_path / "original"), str(tmp_path / "back"))


def test_derived_files_that_were_there_are_refreshed(tmp_path):
    """an annotated anchor's gene files, genome_dist.tsv and the k-mer statistics, all present in the source, are what a
    fresh index of the kept samples with the same switches holds"""
    fx = H.load_case("n9_k21")
    k = int(fx["k"])
    _, allp = _tables(tmp_path, fx, [], {0: _gff_for(fx, 0, tmp_path)})
    switches = dict(genome_dist=True, kmer_stats=True, annotate=True)
    src = _run(allp, tmp_path / "idx", k, **switches)
    for f in ("kmer_shared.tsv", "kmer_occupancy.tsv", "genome_dist.tsv", "anchor/g0/gene.bed.gz", "anchor/g0/bitsum.genes.tsv"):
        assert (src / f).exists(), f
    out = tmp_path / "sub"
    _subset(src, out, drop="g3")
    kept = [f"g{g}" for g in range(9) if g != 3]
    assert "g3" not in (out / "kmer_shared.tsv").read_text().splitlines()[0] and (out / "genome_dist.tsv").read_bytes() != (src / "genome_dist.tsv").read_bytes()
    fresh = _run(_kept_table(tmp_path, allp, kept), tmp_path / "fresh", k, **switches)
    _same_index_payload(str(fresh), str(out))
    # the GFF gone: the annotated anchor cannot be tabulated
    os.replace(tmp_path / "g0.gff", tmp_path / "g0.gff.hidden")
    with pytest.raises(ValueError, match="GFF"):
        _subset(src, tmp_path / "sub2", drop="g3")
    assert not (tmp_path / "sub2").exists()


def test_kmc_databases_that_were_there_are_exported_for_the_kept_samples(tmp_path):
    fx = H.load_case("n9_k21")
    k = int(fx["k"])
    _, allp = _tables(tmp_path, fx, [])
    src = _run(allp, tmp_path / "idx", k, export_kmc=True)
    assert (src / "kmc" / "bitvec0.kmc_pre").exists()
    kept = [f"g{g}" for g in (8, 0, 1, 2, 4, 5, 7)]
    _subset(src, tmp_path / "sub", keep=kept)
    text = (tmp_path / "sub" / "kmc" / "opdef0.txt").read_text()
    assert "g3" not in text and "g6" not in text and str(tmp_path / "sub") in text
    fresh = _run(_kept_table(tmp_path, allp, kept), tmp_path / "fresh", k, export_kmc=True)
    _same_index_payload(str(fresh), str(tmp_path / "sub"))
    _subset(src, tmp_path / "bare", keep=kept, sequence_files=False)
    assert not (tmp_path / "bare" / "kmc").exists()


def test_umap_files_that_were_there_are_made_from_the_new_rows(tmp_path):
    """chrom_umaps.csv and genome_umap.csv of a kept anchor are afterwards what a fresh index of the kept samples with the same
    settings holds (their input is the pair counts of the kept samples' columns): no sequence is needed for them"""
    from panagram_amd import index as pidx
    k, lens, nbin = 21, [60_000, 61_300, 58_100], 2000
    gen = po.synth_genomes(4, lens, 0.02, 23)
    rows = []
    for g in range(4):
        fa = tmp_path / f"g{g}.fa"
        fa.write_bytes(po.fasta_text([f"chr{i + 1}" for i in range(len(lens))], [po.codes_to_ascii(c) for c in gen[g]]))
        rows.append((f"g{g}", str(fa), g == 0))
    for nm, part in (("all", rows), ("kept", [rows[0], rows[3], rows[1]])):
        pd.DataFrame(part, columns=["name", "fasta", "anchor"]).to_csv(tmp_path / f"{nm}.tsv", sep="\t", index=False)
    settings = dict(k=k, chrom_umap=pidx.UMAP(bin_size=nbin), genome_umap=pidx.UMAP(bin_size=nbin), umaps=True)
    src, fresh = tmp_path / "idx", tmp_path / "fresh"
    pidx.Index(str(tmp_path / "all.tsv"), prefix=str(src), **settings).run()
    pidx.Index(str(tmp_path / "kept.tsv"), prefix=str(fresh), **settings).run()
    for g in range(4):
        os.replace(tmp_path / f"g{g}.fa", tmp_path / f"g{g}.hidden")
    assert _subset(src, tmp_path / "sub", keep="g0,g3,g1") == ["rewrote anchor g0: 4 -> 3 samples"]
    for f in ("chrom_umaps.csv", "genome_umap.csv"):
        got = (tmp_path / "sub" / "anchor" / "g0" / f).read_bytes()
        assert got == (fresh / "anchor" / "g0" / f).read_bytes(), f
        assert got != (src / "anchor" / "g0" / f).read_bytes(), f
    _same_index_payload(str(fresh), str(tmp_path / "sub"))


def test_no_sequence_is_read(tmp_path):
    """with every FASTA hidden: a plain index subsets fine; one with genome_dist.tsv is refused, the file named, and goes
    through without that file under sequence_files=False"""
    fx = H.load_case("n9_k21")
    k = int(fx["k"])
    _, allp = _tables(tmp_path, fx, [])
    kept = [f"g{g}" for g in (4, 0, 6, 2)]
    plain = _run(allp, tmp_path / "plain", k)
    withdist = _run(allp, tmp_path / "withdist", k, genome_dist=True)
    fresh = _run(_kept_table(tmp_path, allp, kept), tmp_path / "fresh", k)
    for g in range(9):
        os.replace(tmp_path / f"g{g}.fa", tmp_path / f"g{g}.hidden")
    _subset(plain, tmp_path / "sub", keep=kept)
    _same_index_payload(str(fresh), str(tmp_path / "sub"))
    before = _tree_bytes(withdist)
    with pytest.raises(ValueError, match=r"genome_dist\.tsv.*g4\.fa"):
        _subset(withdist, tmp_path / "sub2", keep=kept)
    assert not (tmp_path / "sub2").exists() and _tree_bytes(withdist) == before
    _subset(withdist, tmp_path / "sub2", keep=kept, sequence_files=False)
    assert not (tmp_path / "sub2" / "genome_dist.tsv").exists()
    _same_index_payload(str(fresh), str(tmp_path / "sub2"))


def test_refusals_and_failures_leave_nothing_behind(tmp_path, monkeypatch):
    from panagram_amd import engine, index as pidx
    fx = H.load_case("n9_k21")
    _, allp = _tables(tmp_path, fx, [])
    src = _run(allp, tmp_path / "idx", int(fx["k"]))
    before = _tree_bytes(src)
    out = tmp_path / "sub"

    def refused(match, out_dir=out, index_kw=None, **kw):
        idx = pidx.Index(str(src), mode="r", **(index_kw or {}))
        try:
            with pytest.raises(ValueError, match=match):
                idx.subset(str(out_dir), **kw)
        finally:
            idx.close()
        assert _tree_bytes(src) == before
        assert not out.exists()

    refused("no such sample.*g9", keep="g0,g9")
    refused("no such sample", drop="nobody")
    refused("twice.*g1", keep="g1,g0,g1")
    refused("one of", keep="g0", drop="g1")
    refused("one of")
    refused("nothing kept", drop=",".join(f"g{g}" for g in range(9)))
    refused("no kept anchor.*g1", keep="g0,g1", anchors="g1")    # kept, but no anchor
    refused("no kept anchor.*g4", keep="g0,g1", anchors="g4")    # an anchor, but not kept
    refused("one process", drop="g8", index_kw=dict(world=2))
    refused("itself or lies inside", out_dir=src, drop="g8")
    refused("itself or lies inside", out_dir=src / "anchor" / "new", drop="g8")
    full = tmp_path / "full"
    full.mkdir()
    (full / "something").write_text("x")
    refused("not empty", out_dir=full, drop="g8")
    assert os.listdir(full) == ["something"]
    # a kept anchor's inputs gone (put back each time); a dropped anchor's do not matter
    for fname in ("bitmap.1.gz", "bitmap.1.gzi", "chrs.tsv"):
        victim = src / "anchor" / "g4" / fname
        os.replace(victim, str(victim) + ".hidden")
        try:
            idx = pidx.Index(str(src), mode="r")
            try:
                with pytest.raises(ValueError, match=fname.replace(".", r"\.")):
                    idx.subset(str(out), drop="g8")
            finally:
                idx.close()
            assert not out.exists()
            if fname == "bitmap.1.gz":
                _subset(src, tmp_path / "without_g4", drop="g4")
        finally:
            os.replace(str(victim) + ".hidden", victim)
        assert _tree_bytes(src) == before
    # the rows do not fit: nothing is left of the new directory
    with monkeypatch.context() as m:
        m.setattr(engine.Context, "mem_info", lambda self: (64 << 20, 1 << 38))
        idx = pidx.Index(str(src), mode="r")
        try:
            with pytest.raises(MemoryError, match="free"):
                idx.subset(str(out), drop="g8")
        finally:
            idx.close()
    assert not out.exists() and _tree_bytes(src) == before
    # an empty directory is taken
    out.mkdir()
    assert _subset(src, out, drop="g8") == _lines(fx, list(range(8)))


def test_subset_cli(tmp_path, capsys):
    from panagram_amd.__main__ import main
    fx = H.load_case("n9_k21")
    k = int(fx["k"])
    _, allp = _tables(tmp_path, fx, [])
    src = _run(allp, tmp_path / "idx", k)
    capsys.readouterr()
    assert main(["subset", str(src), "-o", str(tmp_path / "sub"), "--keep", "g8,g0,g3", "--anchors", "g8"]) == 0
    assert capsys.readouterr().out.splitlines() == ["dropped anchor g0", "dropped anchor g4", "rewrote anchor g8: 9 -> 3 samples"]
    fresh = _run(_kept_table(tmp_path, allp, ["g8", "g0", "g3"], anchors=["g8"]), tmp_path / "fresh", k)
    _same_index_payload(str(fresh), str(tmp_path / "sub"))
    assert main(["subset", str(src), "-o", str(tmp_path / "sub3"), "--drop", "g1", "--no-sequence-files"]) == 0
    with pytest.raises(SystemExit):
        main(["subset", str(src), "-o", str(tmp_path / "sub2"), "--keep", "g8", "--drop", "g0"])
    assert not (tmp_path / "sub2").exists()
