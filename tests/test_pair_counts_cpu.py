"""CPU: the host side of the region tree — which rows Genome.pair_counts hands to the engine (exactly query()'s), its
budgeted pieces, Index.region_tree's linkage / order / Newick / shared_pct and its edge cases, the `tree` subcommand —
with a numpy stand-in for the rows container (tests/pairs_ref.py computes what k_pair_counts would) and an in-memory
payload in place of the bitmap files."""
import re
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest

from panagram_amd import index as pidx
from tests import rows_craft as rc
from tests.pairs_ref import ref_pair_counts

LOW = 100
SIZES = {"c1": 1234, "c2": 777, "c3": 1}


class _Region:
    """stands in for the rows container of one region: payload rows [row0, row0 + nrows) of bitmap.<bstep>"""

    def __init__(self, payload, n, bstep, row0, nrows, log):
        assert 0 <= row0 and nrows >= 1 and row0 + nrows <= len(payload), "the region leaves the file"
        self.rows, self.n, self.bstep = payload[row0:row0 + nrows], n, bstep
        log.append((bstep, row0, nrows))

    def pair_counts(self, contigs, starts, ends, step, stride):
        assert step == self.bstep and list(contigs) == [0] * len(starts)
        for e in ends:  # every sampled row inside the contig, as the C ABI demands
            assert e == 0 or (int(e) - 1) * stride < len(self.rows)
        return np.stack([ref_pair_counts(self.rows, self.n, s, e, stride) for s, e in zip(starts, ends)]).astype(np.uint64)

    def close(self):
        pass


class _Idx(pidx.Index):
    def close(self):
        pass


def _scene(monkeypatch, n, sizes=SIZES, density=0.5, seed=5):
    """(index, genome, log of the regions read): an index of n genomes whose one anchor's bitmaps live in memory"""
    rng = np.random.default_rng(seed)
    names = pd.Index([f"g{i}" for i in range(n)], name="name")
    full = {c: rc.pack(rng.random((s, n)) < density) for c, s in sizes.items()}
    payload = {1: np.concatenate(list(full.values())), LOW: np.concatenate([r[::LOW] for r in full.values()])}
    idx = object.__new__(_Idx)
    idx.samples, idx.lowres_step = pd.DataFrame(index=names), LOW
    g = object.__new__(pidx.Genome)
    g.index, g.name, g.ngenomes, g.nbytes, g.steps = idx, "g0", n, rc.row_bytes(n), [1, LOW]
    g.prefix = "/nowhere"
    g.set_chrs(pd.DataFrame({"size": list(sizes.values())}, index=pd.Index(list(sizes), name="name")))
    g.blocks = {1: None, LOW: None}
    idx.genomes = {"g0": g}
    by_file = {g.bitmap_gz_fname(s): p for s, p in payload.items()}
    monkeypatch.setattr(pidx, "bgzf_read", lambda path, blocks, b0, length: by_file[path].reshape(-1)[b0:b0 + length].tobytes())
    log = []
    g._rows_region = lambda bstep, row0, nrows: _Region(payload[bstep], n, bstep, row0, nrows, log)
    return idx, g, log


def _btb(frame):
    b = frame.to_numpy().astype(np.int64)
    return b.T @ b


REGIONS = [("c1", None, None), ("c1", 13, 1001), ("c1", 150, 1234), ("c2", 250, 777), ("c2", 5, 6), ("c2", 299, 301), ("c3", None, None)]


@pytest.mark.parametrize("step", [1, 7, 100, 300])
def test_pair_counts_selects_querys_rows(monkeypatch, step):
    """steps read from bitmap.1 (1, 7) and from the low-resolution bitmap (100, 300); starts and ends off the step's
    multiples, an end equal to the chromosome's size, a region of one row"""
    idx, g, log = _scene(monkeypatch, 11)
    one_row = 0
    for chrom, start, end in REGIONS:
        q = g.query(chrom, start, end, step)
        got = g.pair_counts(chrom, start, end, step)
        assert list(got.index) == list(idx.genome_names) and list(got.columns) == list(idx.genome_names)
        assert got.to_numpy().dtype.kind == "i"
        assert np.array_equal(got.to_numpy(), _btb(q)), (chrom, start, end, step)
        assert np.array_equal(idx.pair_counts("g0", chrom, start, end, step).to_numpy(), got.to_numpy())
        one_row += len(q) == 1
    assert one_row >= 2
    whole = g.pair_counts(step=step)  # chrom=None: the sum over the chromosomes
    assert np.array_equal(whole.to_numpy(), sum(_btb(g.query(c, None, None, step)) for c in SIZES))


@pytest.mark.parametrize("step,rows_per_piece", [(7, 50), (1, 97), (300, 5), (300, 4)])
def test_tiny_budget_keeps_the_sampling_phase(monkeypatch, step, rows_per_piece):
    """a budget of a few rows cuts the region into pieces whose length the stride does not divide: the same matrix"""
    idx, g, log = _scene(monkeypatch, 11)
    bstep = LOW if step % LOW == 0 else 1
    stride = step // bstep
    assert rows_per_piece % stride or stride == 1
    want = g.pair_counts("c1", 3, 1230, step)
    assert len(log) == 1
    g.similarity_budget = rows_per_piece * g.nbytes * bstep
    got = g.pair_counts("c1", 3, 1230, step)
    assert len(log) - 1 >= 3
    assert all(nrows <= rows_per_piece for _, _, nrows in log[1:])
    assert np.array_equal(got.to_numpy(), want.to_numpy()) and np.array_equal(want.to_numpy(), _btb(g.query("c1", 3, 1230, step)))


def test_pair_counts_input_errors(monkeypatch):
    idx, g, log = _scene(monkeypatch, 3)
    with pytest.raises(KeyError, match="no chromosome"):
        g.pair_counts("nope")
    with pytest.raises(ValueError, match="step"):
        g.pair_counts("c1", step=0)
    with pytest.raises(ValueError, match="need a chromosome"):
        g.pair_counts(None, 5, 10)


# ---------------------------------------------------------------------------
# region_tree
# ---------------------------------------------------------------------------
def _parse(newick):
    """Newick text -> (leaf names in written order, [(frozenset of leaves, branch length or None)] of the internal nodes,
    {leaf: branch length text})"""
    assert newick.endswith(";")
    pos, internals, leaf_len, leaves = 0, [], {}, []

    def node():
        nonlocal pos
        if newick[pos] == "(":
            pos += 1
            under = set()
            while True:
                under |= node()
                if newick[pos] == ",":
                    pos += 1
                    continue
                assert newick[pos] == ")"
                pos += 1
                break
            m = re.match(r":(-?\d+\.\d+)", newick[pos:])
            internals.append((frozenset(under), m.group(1) if m else None))
            pos += len(m.group(0)) if m else 0
            return under
        m = re.match(r"([^:(),;]+):(-?\d+\.\d+)", newick[pos:])
        assert m, newick[pos:pos + 20]
        pos += len(m.group(0))
        leaves.append(m.group(1))
        leaf_len[m.group(1)] = m.group(2)
        return {m.group(1)}

    node()
    assert newick[pos:] == ";"
    return leaves, internals, leaf_len


@pytest.mark.parametrize("n", [2, 3, 11, 40])
def test_region_tree_equals_scipy_on_the_bitmap(monkeypatch, n):
    hier = pytest.importorskip("scipy.cluster.hierarchy")
    idx, g, log = _scene(monkeypatch, n, density=0.3, seed=n)
    names = list(idx.genome_names)
    for chrom, start, end, step in [("c1", 13, 1001, 1), ("c1", None, None, None), ("c2", 100, 700, 7)]:
        t = idx.region_tree("g0", chrom, start, end, step)
        q = g.query(chrom, start, end, LOW if step is None else step)  # (the default step: the low-resolution one)
        bits = q.to_numpy().astype(np.float64)
        Z = hier.linkage(bits.T, "ward", "euclidean")
        assert np.array_equal(t.linkage, Z)
        assert np.array_equal(t.counts.to_numpy(), _btb(q))
        H = (bits[:, :, None] != bits[:, None, :]).sum(axis=0)
        assert np.array_equal(t.distance.to_numpy(), H) and t.distance.to_numpy().dtype.kind == "i"
        d = np.diag(t.counts.to_numpy())
        assert np.allclose(t.shared_pct.to_numpy(), d / d.max() * 100) and list(t.shared_pct.index) == names
        # order and the leaves under every internal node: scipy's tree
        root, nodes = hier.to_tree(Z, rd=True)
        assert t.order == [names[i] for i in root.pre_order()] == [names[i] for i in hier.leaves_list(Z)]
        leaves, internals, leaf_len = _parse(t.newick)
        assert sorted(leaves) == sorted(names)
        want_sets = {frozenset(names[i] for i in nd.pre_order()) for nd in nodes if not nd.is_leaf()}
        assert {s for s, _ in internals} == want_sets and len(internals) == n - 1
        # branch lengths: parent height - node height, to two decimals; the root has none
        parent = {}
        for nd in nodes:
            if not nd.is_leaf():
                parent[nd.left.id], parent[nd.right.id] = nd, nd
        by_set = {frozenset(names[i] for i in nd.pre_order()): nd for nd in nodes}
        for s, length in internals:
            nd = by_set[s]
            if nd is root:
                assert length is None
            else:
                assert length == "%.2f" % (parent[nd.id].dist - nd.dist)
        for i, nm in enumerate(names):
            assert leaf_len[nm] == "%.2f" % parent[i].dist
        # the viewer's writer puts a node's right child first (view.py:593-595)
        assert t.newick.startswith("(") and t.newick.endswith(");")
        first_written = set()
        right = frozenset(names[i] for i in root.right.pre_order())
        for nm in leaves:
            first_written.add(nm)
            if len(first_written) == len(right):
                break
        assert first_written == right


def test_region_tree_all_zero_region(monkeypatch):
    pytest.importorskip("scipy")
    idx, g, log = _scene(monkeypatch, 5, density=0.0)
    t = idx.region_tree("g0", "c1", 0, 500, 1)
    assert not t.counts.to_numpy().any() and not t.distance.to_numpy().any()
    assert list(t.shared_pct) == [0.0] * 5 and not t.shared_pct.isna().any()
    assert sorted(_parse(t.newick)[0]) == sorted(idx.genome_names)


def test_region_tree_one_and_two_genomes(monkeypatch):
    idx, g, log = _scene(monkeypatch, 1, density=0.7)
    t = idx.region_tree("g0", "c1")
    assert t.newick == "(g0:0.00);" and t.order == ["g0"] and t.linkage.shape == (0, 4)
    assert t.counts.shape == (1, 1) and t.counts.iloc[0, 0] == int(g.query("c1", None, None, LOW)["g0"].sum())
    assert t.shared_pct["g0"] == 100.0
    pytest.importorskip("scipy")
    idx, g, log = _scene(monkeypatch, 2, density=0.5)
    t = idx.region_tree("g0", "c1", step=1)
    h = float(np.sqrt(t.distance.iloc[0, 1]))
    assert t.linkage.shape == (1, 4) and t.linkage[0, 2] == h
    assert t.newick == "(g1:%.2f,g0:%.2f);" % (h, h) and t.order == ["g0", "g1"]


def test_region_tree_empty_region_raises(monkeypatch):
    idx, g, log = _scene(monkeypatch, 4)
    with pytest.raises(ValueError, match=r"c2:300-300"):
        idx.region_tree("g0", "c2", 300, 300, 1)
    with pytest.raises(ValueError, match=r"c2:500-400"):
        idx.region_tree("g0", "c2", 500, 400)


def test_region_tree_without_scipy(monkeypatch):
    import sys
    idx, g, log = _scene(monkeypatch, 4)
    monkeypatch.setitem(sys.modules, "scipy.cluster.hierarchy", None)
    with pytest.raises(ImportError, match="needs scipy"):
        idx.region_tree("g0", "c1")
    assert g.pair_counts("c1").shape == (4, 4)  # (the counts do not need it)


# ---------------------------------------------------------------------------
# the subcommand
# ---------------------------------------------------------------------------
def test_cli_tree_and_matrix(monkeypatch, tmp_path, capsys):
    pytest.importorskip("scipy")
    from panagram_amd.__main__ import main
    idx, g, log = _scene(monkeypatch, 9)
    opened = []

    def open_index(path, mode=None, device=0):
        opened.append((path, mode, device))
        return idx
    monkeypatch.setattr(pidx, "Index", open_index)
    out = tmp_path / "m.tsv"
    assert main(["tree", "some/index", "g0", "c1", "13", "1001", "7", "--matrix", str(out), "--device", "0"]) == 0
    assert opened == [("some/index", "r", 0)]
    newick = capsys.readouterr().out.strip()
    want = idx.region_tree("g0", "c1", 13, 1001, 7)
    assert newick == want.newick and sorted(_parse(newick)[0]) == sorted(idx.genome_names)
    lines = out.read_text().splitlines()
    names = list(idx.genome_names)
    assert lines[0].split("\t")[1:] == names and len(lines) == 1 + len(names)
    for nm, line in zip(names, lines[1:]):
        cells = line.split("\t")
        assert cells[0] == nm and [int(c) for c in cells[1:]] == list(want.counts.loc[nm]) and all(re.fullmatch(r"\d+", c) for c in cells[1:])
    # --whole: the genome-wide sum, at the default (low-resolution) step
    assert main(["tree", "some/index", "g0", "--whole", "--matrix", str(out)]) == 0
    assert capsys.readouterr().out.strip() == pidx.RegionTree.from_counts(g.pair_counts(step=LOW), names).newick
    got = pd.read_csv(out, sep="\t", index_col=0)
    assert np.array_equal(got.to_numpy(), g.pair_counts(step=LOW).to_numpy())
    for bad in (["tree", "some/index", "g0"], ["tree", "some/index", "g0", "c1", "--whole"]):
        with pytest.raises(SystemExit):
            main(bad)


# ---------------------------------------------------------------------------
# the restatement itself
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 8, 9, 33, 130])
@pytest.mark.parametrize("stride", [1, 3])
def test_ref_diagonal_is_the_column_sums(n, stride):
    """ties tests/pairs_ref.py to the column-sum restatement the suite already trusts (rows_craft.ref_bin_colsums, itself
    tied to bitmap_to_bins), bits past N planted and ignored"""
    rows = rc.with_pad_bits(rc.dense(700, n, 9), n)
    ns = (len(rows) - 1) // stride + 1
    for s, e in [(0, ns), (5, 5), (17, 18), (3, ns - 1)]:
        C = ref_pair_counts(rows, n, s, e, stride)
        cs, kept = rc.ref_bin_colsums(rows, n, [s], [e], stride, None, False)
        assert np.array_equal(np.diag(C), cs[0]) and np.array_equal(C, C.T)
        assert C.max(initial=0) <= kept[0] == e - s
        bits = rc.unpack(rows[::stride][s:e], n).astype(bool)
        for a, b in [(0, n - 1), (n // 2, n // 3)]:
            assert C[a, b] == int((bits[:, a] & bits[:, b]).sum())
