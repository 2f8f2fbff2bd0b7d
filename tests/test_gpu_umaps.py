"""GPU: chrom_umaps.csv and genome_umap.csv (Genome.write_umaps) on an index written by Index.run(): the input matrix against
the reference's pandas expression on the rows read back on the host, the neighbour table against tests/knn_ref.py, the files
as the viewer reads them (view.py:922, 2197), and a planted two-group matrix through run_umap."""
import os

import numpy as np
import pandas as pd
import pytest

from oracle import pyoracle as po
from tests import knn_ref
from tests.test_gpu_intros import write_samples

pytestmark = pytest.mark.gpu

K = 21
LENS = [60_000, 61_300, 58_100]
BIN = 2000
HEADER_CHROM = "chrom,start,end,umap1,umap2,cluster"


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


@pytest.fixture(scope="module")
def samples(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("umaps_src")
    chroms = [f"chr{i + 1}" for i in range(len(LENS))]
    return write_samples(tmp, po.synth_genomes(4, LENS, 0.02, 23), [f"g{i}" for i in range(4)], chroms)


@pytest.fixture(scope="module")
def built(samples, tmp_path_factory):
    from panagram_amd import index as pidx
    out = str(tmp_path_factory.mktemp("umaps_idx") / "idx")
    pidx.Index(samples, prefix=out, k=K, anchor_genomes=["g0"], chrom_umap=pidx.UMAP(bin_size=BIN),
               genome_umap=pidx.UMAP(bin_size=BIN)).run()
    return out, _files(out)


def _want_matrix(idx, g):
    return pd.concat({c: idx.bitmap_to_paircount_bins(idx.query_bitmap("g0", c, step=idx.lowres_step), BIN).T.fillna(0)
                      for c in g.chrs.index}, names=["chrom", "start"])


def test_input_matrix_and_neighbours(built):
    from panagram_amd import engine, index as pidx, umap
    out, _ = built
    idx = pidx.Index(out, mode="r")
    try:
        g = idx["g0"]
        assert idx.chrom_umap.bin_size == BIN and idx.genome_umap.bin_size == BIN  # (carried through config.yaml)
        frame, X = umap.paircount_matrix(g, BIN)
        want = _want_matrix(idx, g)
        assert len(X) == sum(-(-n // BIN) for n in g.chrs["size"]) and X.shape[1] == 4
        assert np.array_equal(X, want.to_numpy().astype(np.float32))
        assert list(zip(frame["chrom"], frame["start"])) == list(want.index)
        c = frame["chrom"].to_numpy()
        seg = np.concatenate([[0], np.flatnonzero(c[1:] != c[:-1]) + 1, [len(c)]])
        assert len(seg) == 4
        for k, s in ((4, seg), (4, None), (9, seg)):
            gi, gd = engine.knn_rows(idx.context, X, k, s)
            wi, wd = knn_ref.knn_rows(X, k, s)
            assert np.array_equal(gi, wi) and np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), (k, s is None)
    finally:
        idx.close()


def test_write_umaps(built):
    from panagram_amd import index as pidx
    out, before = built
    idx = pidx.Index(out, mode="r")
    try:
        g = idx["g0"]
        fc, fg = g.write_umaps()
        assert (fc, fg) == (g.chrom_umaps_filename, g.genome_umap_filename)
        first = open(fc, "rb").read(), open(fg, "rb").read()
        assert first[0].split(b"\n")[0].decode() == HEADER_CHROM and first[1].split(b"\n")[0].decode() == HEADER_CHROM
        assert sorted(set(_files(out)) - set(before)) == ["anchor/g0/chrom_umaps.csv", "anchor/g0/genome_umap.csv"]
        g.load_umaps()
        nbins = {c: -(-int(n) // BIN) for c, n in g.chrs["size"].items()}
        assert len(g.chrom_umaps) == len(g.genome_umap) == sum(nbins.values())
        for frame_of in (lambda c: g.chrom_umaps.loc[c], lambda c: g.genome_umap.query("chrom == @c")):  # view.py:922, 2197
            for c, nb in nbins.items():
                part = frame_of(c)
                assert len(part) == nb and list(part["start"]) == list(range(0, nb * BIN, BIN))
                assert (part["end"] - part["start"] == BIN).all()
                assert np.isfinite(part[["umap1", "umap2"]].to_numpy(np.float64)).all()
        for c in nbins:  # each chromosome is an embedding of its own: labels from 0, dense
            lab = g.chrom_umaps.loc[c]["cluster"].to_numpy()
            assert lab.dtype.kind == "i" and lab[0] == 0 and set(lab) == set(range(lab.max() + 1))
        lab = g.genome_umap["cluster"].to_numpy()
        assert lab.dtype.kind == "i" and lab[0] == 0 and set(lab) == set(range(lab.max() + 1))
        assert g.chrom_umaps[["umap1", "umap2"]].to_numpy().std() > 0  # (not the fallback's zeros)
        g.write_umaps()
        assert (open(fc, "rb").read(), open(fg, "rb").read()) == first
    finally:
        idx.close()


def test_planted_groups_stay_apart(ctx):
    """two groups of 40 bins whose genomes do not overlap: no DBSCAN label holds bins of both"""
    from panagram_amd import index as pidx, umap
    rng = np.random.default_rng(31)
    X = np.zeros((80, 8), np.float32)
    X[:40, :4] = rng.integers(1, 9, (40, 4)) / 8
    X[40:, 4:] = rng.integers(1, 9, (40, 4)) / 8
    frame = pd.DataFrame({"chrom": ["c1"] * 80, "start": np.arange(80) * BIN})
    out = umap.run_umap(X, frame, pidx.UMAP(bin_size=BIN), ctx=ctx)
    lab = out["cluster"].to_numpy()
    assert np.isfinite(out[["umap1", "umap2"]].to_numpy()).all()
    assert not set(lab[:40]) & set(lab[40:])
    assert out.equals(umap.run_umap(X, frame, pidx.UMAP(bin_size=BIN), ctx=ctx))


def test_index_flag_writes_them_and_default_tree_is_unchanged(samples, tmp_path):
    from panagram_amd.__main__ import main
    plain, flagged = str(tmp_path / "plain"), str(tmp_path / "flagged")
    assert main(["index", samples, "-o", plain, "-k", str(K), "--anchor_genomes", "g0"]) == 0
    assert main(["index", samples, "-o", flagged, "-k", str(K), "--anchor_genomes", "g0", "--umaps"]) == 0
    new = ["anchor/g0/chrom_umaps.csv", "anchor/g0/genome_umap.csv"]
    assert not set(new) & set(_files(plain))
    assert sorted(set(_files(flagged)) - set(_files(plain))) == new and set(_files(plain)) <= set(_files(flagged))
    assert open(os.path.join(plain, "config.yaml")).read() == open(os.path.join(flagged, "config.yaml")).read()
    # the default bin size (100 kb) leaves one bin per chromosome: the reference's fallback rows
    got = pd.read_csv(os.path.join(flagged, new[0]), index_col="chrom")
    assert list(got.index) == ["chr1", "chr2", "chr3"] and (got[["umap1", "umap2", "cluster"]].to_numpy() == 0).all()
    assert main(["umaps", flagged, "g0"]) == 0
