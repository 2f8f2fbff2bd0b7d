"""GPU: k_pair_counts (panagram_amd/csrc/pg_pairs.hip) on rows PLANTED into a rows container (tests/rows_craft.py) and
through the read side on indexes written by Index.run().  Every result is exactly equal to B.T @ B of the rows as 0/1
(tests/pairs_ref.py, tied on the CPU to the column-sum restatement: tests/test_pair_counts_cpu.py).

Which kernel runs for which N: N <= 128 k_pair_counts<4> (the row's words in registers, one slice of 4 x 4 pair blocks);
129 .. 512 k_pair_counts<0> (N = 129, 130: 1 slice of the grid's z; N = 256: 3 slices).  A tile is 256 sampled rows."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from oracle import pyoracle as po
from tests import rows_craft as rc
from tests.pairs_ref import ref_pair_counts

pytestmark = pytest.mark.gpu

K = 21
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS_N = [1, 2, 7, 8, 9, 27, 32, 33, 64, 65, 127, 128, 129, 130, 256]
LIMIT = 512  # PAIRS_MAX_GENOMES (pg_kernels.h)
SEG = 300    # rows of each pattern in contig 0 (a tile and a bit: every pattern crosses a tile boundary)
STRIDES = [1, 3, 100]


def crafted(n):
    """contig 0: ones, zeros, column N - 1, column 0, ramp, checker, dense, SEG rows each (in this order); contig 1: dense"""
    parts = [rc.ones(SEG, n), rc.zeros(SEG, n), rc.column(SEG, n, n - 1), rc.column(SEG, n, 0), rc.ramp(SEG, n),
             rc.checker(SEG, n), rc.dense(SEG, n, 40 + n)]
    return [np.concatenate(parts), rc.dense(1111, n, 41 + n)]


def windows(nks, stride):
    """(contigs, starts, ends) in sampled rows: every pattern of contig 0 on its own (stride 1), an empty window, lengths 1,
    63, 64, 65, 255, 256, 257 from starts that are no multiples of 64, 700 rows (three tiles, the last one partly filled),
    windows ending on each contig's last row, each contig whole"""
    ns = [(nk - 1) // stride + 1 for nk in nks]
    w = [(0, 5, 5), (0, 0, ns[0]), (1, 0, ns[1]), (0, ns[0] - 1, ns[0]), (1, ns[1] - 1, ns[1]), (1, ns[1], ns[1])]
    for i, length in enumerate([1, 63, 64, 65, 255, 256, 257]):
        for c in (0, 1):
            s = min(7 + 37 * i, ns[c] - 1)
            w.append((c, s, min(s + length, ns[c])))
    w += [(0, min(130, ns[0] - 1), min(830, ns[0])), (1, min(411, ns[1] - 1), ns[1])]
    if stride == 1:
        w += [(0, SEG * i, SEG * (i + 1)) for i in range(7)]
    c, s, e = (np.array(x) for x in zip(*w))
    return c.astype(np.uint32), s.astype(np.uint64), e.astype(np.uint64)


def _want(rows, n, contigs, starts, ends, stride):
    return np.stack([ref_pair_counts(rows[c], n, s, e, stride) for c, s, e in zip(contigs, starts, ends)])


@pytest.mark.parametrize("n", PAIRS_N)
def test_pair_counts_on_crafted_rows(ctx, n):
    """every pattern, window length and stride at every word boundary of N and on both kernels; the bytes between and
    behind the contigs' rows hold 0xFF; then the same rows with the bits past N set: nothing changes"""
    rows = crafted(n)
    nks = [len(r) for r in rows]
    padded = [rc.with_pad_bits(r, n) for r in rows] if n % 8 else None
    res = rc.container(ctx, K, n, nks, colsums=False)
    res_pad = rc.container(ctx, K, n, nks, colsums=False) if padded else None
    try:
        rc.plant(res, rows, poison=0xFF)
        res.rows_epilogue()  # (a rows container is read once its statistics have been enqueued)
        if res_pad is not None:
            rc.plant(res_pad, padded, poison=0xFF)
            res_pad.rows_epilogue()
        for stride in STRIDES:
            contigs, starts, ends = windows(nks, stride)
            want = _want(rows, n, contigs, starts, ends, stride)
            got = res.pair_counts(contigs, starts, ends, step=1, stride=stride)
            assert got.shape == (len(contigs), n, n) and got.dtype == np.uint64
            for i in range(len(contigs)):
                assert np.array_equal(got[i].astype(np.int64), want[i]), (n, stride, int(contigs[i]), int(starts[i]), int(ends[i]))
            assert not got[0].any() and not got[5].any()  # the empty windows
            if stride == 1:  # ones: every pair SEG; a single column: one entry
                assert (got[-7] == SEG).all() and not got[-6].any()
                assert got[-5].sum() == SEG == got[-5][n - 1, n - 1] and got[-4].sum() == SEG == got[-4][0, 0]
            if res_pad is not None:
                again = res_pad.pair_counts(contigs, starts, ends, step=1, stride=stride)
                assert np.array_equal(again, got), (n, stride, "bits past N set")
        none = res.pair_counts([], [], [], step=1, stride=1)  # no window: a no-op
        assert none.shape == (0, n, n)
    finally:
        res.close()
        if res_pad is not None:
            res_pad.close()


@pytest.mark.parametrize("n", [9, 128, 130])
def test_twelve_windows_of_two_contigs_in_one_call(ctx, n):
    """overlapping, nested and equal windows of both contigs in ONE launch: each equals its own reference, so no window's
    atomics land in another's matrix"""
    rows = crafted(n)
    nks = [len(r) for r in rows]
    w = [(0, 0, 900), (1, 0, 900), (0, 100, 700), (0, 100, 700), (1, 300, 301), (0, 650, 1500), (1, 1000, 1111), (0, 2099, 2100),
         (1, 5, 600), (0, 299, 601), (1, 0, 1111), (0, 0, 2100)]
    contigs, starts, ends = (np.array(x) for x in zip(*w))
    res = rc.container(ctx, K, n, nks, colsums=False)
    try:
        rc.plant(res, rows, poison=0xFF)
        res.rows_epilogue()
        got = res.pair_counts(contigs, starts, ends, step=1, stride=1)
        want = _want(rows, n, contigs, starts, ends, 1)
        for i in range(len(w)):
            assert np.array_equal(got[i].astype(np.int64), want[i]), (n, w[i])
        assert np.array_equal(got[2], got[3]) and not np.array_equal(got[0], got[1])
    finally:
        res.close()


@pytest.mark.parametrize("n", [8, 128, 129, 256])
def test_window_cut_into_pieces(ctx, n):
    """One window of 8 998 sampled rows alone in its call: pg_result_pair_counts doubles the pieces while a piece would
    still hold more than 4096 rows and the grid has fewer than 4096 blocks — 1 -> 2 -> 4 here (4 x 4096 >= 8 998), so four
    blocks add their counters into the one matrix with atomics; confirmed on a kernel trace of this test, which lists
    k_pair_counts with a grid of y = 4 (and, for N = 256, z = 3 slices).  Then the same rows at stride 2 (4 500 sampled
    rows: 2 pieces)."""
    nk = 9000
    rows = [np.concatenate([rc.dense(nk - 4500, n, 77), rc.ones(4500, n)])]
    res = rc.container(ctx, K, n, [nk], colsums=False)
    try:
        rc.plant(res, rows, poison=0xFF)
        res.rows_epilogue()
        for stride, s, e in [(1, 1, nk - 1), (2, 0, (nk - 1) // 2 + 1)]:
            got = res.pair_counts([0], [s], [e], step=1, stride=stride)
            assert np.array_equal(got[0].astype(np.int64), ref_pair_counts(rows[0], n, s, e, stride)), (n, stride)
    finally:
        res.close()


def test_limit_and_rows_past_the_contig(ctx):
    from panagram_amd._lib import PanagramHipError
    PG_E_INVALID = -1
    res = rc.container(ctx, K, LIMIT + 1, [300], colsums=False)
    try:
        rc.plant(res, [rc.dense(300, LIMIT + 1, 1)])
        res.rows_epilogue()
        with pytest.raises(PanagramHipError, match=f"1 to {LIMIT}") as ei:
            res.pair_counts([0], [0], [300])
        assert ei.value.code == PG_E_INVALID
    finally:
        res.close()
    n = 12
    rows = [rc.dense(300, n, 2), rc.dense(50, n, 3)]
    res = rc.container(ctx, K, n, [300, 50], colsums=False)
    try:
        rc.plant(res, rows)
        res.rows_epilogue()
        for contigs, starts, ends, stride in [([1], [0], [51], 1), ([0], [0], [101], 3), ([0, 1], [0, 40], [300, 60], 1),
                                              ([2], [0], [1], 1), ([0], [9], [8], 1)]:
            with pytest.raises(PanagramHipError) as ei:
                res.pair_counts(contigs, starts, ends, step=1, stride=stride)
            assert ei.value.code == PG_E_INVALID, (contigs, starts, ends, stride)
        with pytest.raises(PanagramHipError) as ei:
            res.pair_counts([0], [0], [10], step=1, stride=0)
        assert ei.value.code == PG_E_INVALID
        # the last sampled row that does fit
        got = res.pair_counts([0, 1], [0, 0], [100, 50], step=1, stride=1)
        assert np.array_equal(got[1].astype(np.int64), ref_pair_counts(rows[1], n, 0, 50, 1))
        got = res.pair_counts([0], [0], [100], step=1, stride=3)
        assert np.array_equal(got[0].astype(np.int64), ref_pair_counts(rows[0], n, 0, 100, 3))
    finally:
        res.close()


# ---------------------------------------------------------------------------
# end to end: indexes written by Index.run()
# ---------------------------------------------------------------------------
LENS = [6000, 2500]


@pytest.fixture(scope="module", params=[9, 33], ids=["N9", "N33"])
def built(request, tmp_path_factory):
    from panagram_amd import index as pidx
    n = request.param
    tmp = tmp_path_factory.mktemp(f"pairs_n{n}")
    chroms = [f"chr{i + 1}" for i in range(len(LENS))]
    lines = ["name\tfasta"]
    for i, g in enumerate(po.synth_genomes(n, LENS, 0.02, 23 + n)):
        fa = tmp / f"g{i}.fa"
        fa.write_bytes(po.fasta_text(chroms, [po.codes_to_ascii(c) for c in g]))
        lines.append(f"g{i}\t{fa}")
    (tmp / "samples.tsv").write_text("\n".join(lines) + "\n")
    out = str(tmp / "idx")
    pidx.Index(str(tmp / "samples.tsv"), prefix=out, k=K, anchor_genomes=["g0"], lowres_step=100).run()
    return out, n


def _btb(frame):
    b = frame.to_numpy().astype(np.int64)
    return b.T @ b


def test_genome_pair_counts_equal_the_queried_bitmap(built):
    from panagram_amd import index as pidx
    out, n = built
    idx = pidx.Index(out, mode="r")
    try:
        g = idx["g0"]
        names = list(idx.genome_names)
        size = int(g.chrs.loc["chr1", "size"])
        for step in (1, 100, 300):
            for chrom, start, end in [("chr1", None, None), ("chr1", 1234, 5678), ("chr2", 77, int(g.chrs.loc["chr2", "size"])),
                                      ("chr1", size - 1, size)]:
                got = idx.pair_counts("g0", chrom, start, end, step)
                assert list(got.index) == names and list(got.columns) == names
                assert np.array_equal(got.to_numpy(), _btb(idx.query_bitmap("g0", chrom, start, end, step))), (chrom, start, end, step)
        # cut into pieces of a few rows: the same
        whole = g.pair_counts("chr1", 1234, 5678, 7)
        g.similarity_budget = 1000 * g.nbytes
        try:
            assert np.array_equal(g.pair_counts("chr1", 1234, 5678, 7).to_numpy(), whole.to_numpy())
        finally:
            del g.similarity_budget
        # the whole genome at step 1: total_paircounts.csv on the diagonal
        total = g.pair_counts()
        counts = pd.read_csv(os.path.join(g.prefix, "total_paircounts.csv"), index_col="name")["count"]
        assert np.array_equal(np.diag(total.to_numpy()), counts.loc[names].to_numpy())
        assert np.array_equal(total.to_numpy(), sum(_btb(g.query(c)) for c in g.chrs.index))
    finally:
        idx.close()


def test_region_tree_equals_scipy_on_the_queried_bitmap(built):
    hier = pytest.importorskip("scipy.cluster.hierarchy")
    from panagram_amd import index as pidx
    out, n = built
    idx = pidx.Index(out, mode="r")
    try:
        for chrom, start, end, step in [("chr1", None, None, None), ("chr1", 1234, 5678, 1), ("chr2", 10, 2000, 7)]:
            t = idx.region_tree("g0", chrom, start, end, step)
            bits = idx.query_bitmap("g0", chrom, start, end, 100 if step is None else step).to_numpy().astype(np.float64)
            Z = hier.linkage(bits.T, "ward", "euclidean")
            assert np.array_equal(t.linkage, Z), (chrom, start, end, step)
            assert t.order == [idx.genome_names[i] for i in hier.leaves_list(Z)]
    finally:
        idx.close()


def test_tree_subcommand_in_a_child_process(built, tmp_path):
    pytest.importorskip("scipy")
    out, n = built
    m = tmp_path / "pairs.tsv"
    p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "panagram_amd", "tree", out, "g0", "chr2", "100", "2400",
                        "1", "--matrix", str(m)], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    newick = p.stdout.strip().splitlines()[-1]
    assert newick.startswith("(") and newick.endswith(");")
    import re
    leaves = re.findall(r"[(,]([^:(),;]+):\d+\.\d\d", newick)
    assert sorted(leaves) == sorted(f"g{i}" for i in range(n))
    got = pd.read_csv(m, sep="\t", index_col=0)
    assert list(got.index) == list(got.columns) == [f"g{i}" for i in range(n)]
    from panagram_amd import index as pidx
    idx = pidx.Index(out, mode="r")
    try:
        assert np.array_equal(got.to_numpy(), _btb(idx.query_bitmap("g0", "chr2", 100, 2400, 1)))
    finally:
        idx.close()
