"""GPU: engine.novel_runs (k_novel_runs) — the maximal runs of novel k-mer positions along the contigs of an assembly, with what
stands on either side of each — against the numpy model (tests/novel_ref.py), exactly: the crafted contigs (runs at a contig's start
and end, across a tile and a chunk edge, cut by N, with each of the four pairs of neighbours, a substitution, an insertion, a
deletion) at every front end of the pan table's placement and every layout of its lines, a set of 1025 contigs, and the capacity
protocol.

At k = 6 the runs are held to the model exactly as at every k, but that the planted substitution, insertion and deletion give
``bases`` of 1, L and 0 is asserted (tests/test_novel_cpu.py) from k = 21 on only (``novel_ref.EXACT_FROM_K``): among 2080 canonical
6-mers a chance hit splits a planted run.  The runs that cross a tile and a chunk edge, start and end a contig and have no held
neighbour are homopolymer runs and certain at every k."""
import numpy as np
import pytest

from tests import copies_ref as CR
from tests import many_contigs as MC
from tests import novel_ref as NR

pytestmark = pytest.mark.gpu

K, MIN_COUNT, WIDTHS, pan_table = NR.GPU_K, NR.GPU_MIN_COUNT, NR.GPU_WIDTHS, NR.pan_table


def same_runs(got, ref, tag):
    for g, r, what, dt in zip(got[:5], ref[:5], ("contig", "start", "end", "left_held", "right_held"), (np.uint32,) * 3 + (np.uint8,) * 2):
        assert g.dtype == dt and len(g) == len(r), (tag, what, len(g), len(r))
        bad = np.flatnonzero(g.astype(np.int64) != r)
        assert len(bad) == 0, (tag, what, len(bad), bad[:6].tolist(), g[bad[:6]].tolist(), r[bad[:6]].tolist())
    assert tuple(got[5:7]) == tuple(ref[5:7]), (tag, "windows, novel windows", got[5:7], ref[5:7])


def run_crafted(ctx, tbl, k, tag):
    from panagram_amd import engine, novel as nov
    table, _, R, p = NR.crafted(k, MIN_COUNT)
    ref = NR.runs(table, R, k)
    assert len(ref[0]) >= 13 and ref[6] == int((ref[2] - ref[1]).sum())
    ss = engine.SeqSet.from_host(ctx, R)
    try:
        got = engine.novel_runs(tbl, ss)
        same_runs(got, ref, tag)
        assert engine.novel_last_timing()["runs_ms"] > 0
        assert nov.run_bases(*got[1:5], k).tolist() == NR.bases(*ref[1:5], k).tolist()
        # the capacity protocol: the first `cap` runs in (contig, start) order, the full numbers always
        for cap in (0, 5, len(ref[0]), len(ref[0]) + 3):
            part = engine.novel_runs(tbl, ss, cap=cap)
            assert part[5:] == (ref[5], ref[6], len(ref[0])), (tag, cap, part[5:])
            n = min(cap, len(ref[0]))
            for g, r in zip(part[:5], ref[:5]):
                assert len(g) == cap and g[:n].astype(np.int64).tolist() == r[:n].tolist() and not g[n:].any(), (tag, cap)
    finally:
        ss.close()


@pytest.mark.parametrize("n", WIDTHS)
def test_crafted_contigs_at_every_layout(ctx, n):
    keys = NR.crafted(K, MIN_COUNT)[0]
    kw = dict(expected_keys=int(len(keys) * 1.02) + 64, keys_per_line=1.25) if n == 8 else {}
    tbl = pan_table(ctx, K, n, keys, **kw)
    try:
        run_crafted(ctx, tbl, K, n)
    finally:
        tbl.close()


@pytest.mark.parametrize("k", [6, 31, 32])
def test_crafted_contigs_at_every_front_end_of_the_placement(ctx, k):
    tbl = pan_table(ctx, k, 8, NR.crafted(k, MIN_COUNT)[0])
    try:
        run_crafted(ctx, tbl, k, ("k", k))
    finally:
        tbl.close()


def test_a_set_of_1025_contigs(ctx):
    """a fragmented assembly against the table of a diverged copy of it: contigs without a k-mer position at the set's start, in
    its middle and at its end, contigs of one and two positions, N and lower case; the table built from sequence"""
    from panagram_amd import engine
    frags, other = MC.genomes(2, K, MC.COUNTS[0], 11, 1024, d=0.02)
    keys = np.unique(CR.valid_keys(other, K))
    ref = NR.runs(keys, frags, K)
    assert len(frags) == 1025 and len(ref[0]) > 2000 and 0 < ref[6] < ref[5]
    tbl = engine.PanTable(ctx, K, 2)
    so, sf = engine.SeqSet.from_host(ctx, other), engine.SeqSet.from_host(ctx, frags)
    try:
        tbl.insert_seqset(1, so)
        assert tbl.stats()["nkeys"] == len(keys)
        same_runs(engine.novel_runs(tbl, sf), ref, "1025 contigs")
        part = engine.novel_runs(tbl, sf, cap=1000)  # (a cap below the run count, inside a contig's runs)
        assert part[5:] == (ref[5], ref[6], len(ref[0]))
        for g, r in zip(part[:5], ref[:5]):
            assert g.astype(np.int64).tolist() == r[:1000].tolist()
        # the assembly the table was built from holds nothing novel; an empty set none either
        assert [len(x) for x in engine.novel_runs(tbl, so)[:5]] == [0] * 5 and engine.novel_runs(tbl, so)[6] == 0
        none = engine.SeqSet.from_host(ctx, [b"ACGT", b""])
        try:
            assert engine.novel_runs(tbl, none)[5:] == (0, 0)
        finally:
            none.close()
        lib = ctx._lib
        assert lib.pg_novel_runs(tbl._h, sf._h, 0, *[None] * 5, None, None, None) == -1 and b"NULL" in lib.pg_last_error()
        assert lib.pg_novel_runs(tbl._h, sf._h, 4, *[None] * 5, *[None] * 3) == -1
    finally:
        so.close()
        sf.close()
        tbl.close()
