"""k_probe's six-byte queue entries and its units of work against the oracle.

A queue entry of k_probe is (group, position): the line of every overflow level is derived from the group (and, past the
group's own lines, from the key) again.  The cases were laid out for waves that take a SPAN of two neighbouring tiles
(2048 positions) as one unit — measured and not adopted: profiles/span2_ab.txt — and hold for the tile as well.  What can
go wrong sits at the edges: contigs of exactly one / two / three tiles and one position more, N across position 2047,
pieces of the co-schedule of one, two and three tiles, launches over contig ranges and over chunks of the launch order,
a queue that fills in the middle of a unit, chains past the group's own lines.  Bit-exact, as everywhere."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

# k-mers per contig: none (20 bases), one, a tile, a tile + 1, a span, a span + 1, three tiles, five tiles less a bit
NKMERS = [0, 1, 1024, 1025, 2048, 2049, 3072, 5000]
WITH_N = (5, 7)  # the contigs of 2049 and 5000 k-mers carry a stretch of N across position 2047


def _lens(k):
    return [20 if nk == 0 else nk + k - 1 for nk in NKMERS]


@functools.lru_cache(maxsize=None)
def _edge_case(n, k):
    """genomes (ASCII contigs), the oracle's tables, and the oracle's outputs for every contig of every anchored genome"""
    gen = po.synth_genomes(n, _lens(k), 0.03, 4100 + n)
    genomes = [[bytearray(po.codes_to_ascii(c)) for c in g] for g in gen]
    for g in range(n):
        for ci in WITH_N:
            lo = 2040 + g % 3  # (the k-mers at positions lo - k + 1 .. 2055 have no row bits: the end of one tile and the start of the next)
            genomes[g][ci][lo:2056] = b"N" * (2056 - lo)
    genomes = [[bytes(c) for c in g] for g in genomes]
    dbs = po.build_bitvec_dbs(genomes, k)
    anchors = sorted({0, n // 2, n - 1})
    oracle = {}
    for g in anchors:
        for ci, seq in enumerate(genomes[g]):
            if len(seq) >= k:
                oracle[(g, ci)] = _oracle_contig(dbs, seq, k, n)
    return genomes, dbs, anchors, oracle


def _oracle_contig(dbs, seq, k, n):
    """po.anchor_contig; a contig of fewer than 100 k-mers (the oracle's bin length is nkmers // 100) gets its rows from the
    oracle over the contig with a tail of bases behind it — a row depends on its own k-mer alone — and the statistics of
    those rows in bins of one row, the library's rule (bin length at least 1)"""
    nk = len(seq) - k + 1
    if nk >= 100:
        o_rows, o_rows100, o_bins, _, o_cs = po.anchor_contig(dbs, seq, k, n)
        return o_rows, o_rows100, o_bins, o_cs
    o_rows = po.anchor_contig(dbs, seq + b"ACGT" * 40, k, n)[0][:nk]
    bits = np.unpackbits(o_rows, axis=1, bitorder="little")[:, :n]
    popc = bits.sum(axis=1, dtype=np.int64)
    o_bins = np.zeros((nk, n + 1), np.int64)
    o_bins[np.arange(nk), popc] = 1
    return o_rows, o_rows[::100], o_bins, bits.sum(axis=0, dtype=np.int64)


def _table(ctx, genomes, k, n, m=None):
    from panagram_amd import engine
    tbl = engine.PanTable(ctx, k, n)
    if m is not None:
        tbl.set_minimizer(m)
    for g in range(n):
        ss = engine.SeqSet.from_host(ctx, genomes[g])
        tbl.insert_seqset(g, ss)
        ss.close()
    return tbl


def _check_result(res, order, oracle, tag, stats=True):
    """every contig of the result (order[i] = (genome, contig) of the result's contig i) against the oracle"""
    ccs = res.contig_colsums().astype(np.int64) if stats else None
    for i, key in enumerate(order):
        rows, rows100, bins, info = res.download(i, want_bitmap100=stats)
        if key not in oracle:
            assert info["nkmers"] == 0, (tag, key)
            continue
        o_rows, o_rows100, o_bins, o_cs = oracle[key]
        assert info["nkmers"] == len(o_rows), (tag, key)
        assert np.array_equal(rows, o_rows), (tag, key)
        if stats:
            assert np.array_equal(rows100, o_rows100), (tag, key)
            assert np.array_equal(bins.astype(np.int64), o_bins), (tag, key)
            assert np.array_equal(ccs[i], o_cs), (tag, key)


@pytest.mark.parametrize("n,k,m", [(3, 21, 15), (40, 31, None)])
def test_tile_edges_every_schedule(ctx, n, k, m):
    """one-byte rows (n = 3, the window of 7 m-mers) and two-word rows (n = 40): one result over contigs of 0, 1, 1024, 1025,
    2048, 2049, 3072 and 5000 k-mers of three genomes, in plain order, co-scheduled by group with pieces of 1, 2 and 3
    tiles (odd pieces: a contig's neighbouring tiles end up apart in the launch order), and by class"""
    from panagram_amd import engine
    genomes, dbs, anchors, oracle = _edge_case(n, k)
    tbl = _table(ctx, genomes, k, n, m)
    order = [(g, ci) for g in anchors for ci in range(len(NKMERS))]
    ss = engine.SeqSet.from_host(ctx, [genomes[g][ci] for g, ci in order])
    group = np.repeat(np.arange(len(anchors), dtype=np.uint32), len(NKMERS))
    cls = np.tile(np.arange(len(NKMERS), dtype=np.uint32), len(anchors))
    res = engine.AnchorResult(tbl, ss)
    res.run()
    _check_result(res, order, oracle, "plain")
    for piece in (1, 2, 3):
        res.coschedule(group, piece_tiles=piece)
        res.run()
        _check_result(res, order, oracle, f"pieces of {piece}")
    res.coschedule(group, piece_tiles=2, contig_class=cls)
    res.run()
    _check_result(res, order, oracle, "by class")
    res.coschedule(group, contig_class=cls)
    res.run()
    _check_result(res, order, oracle, "by class, default piece")
    res.coschedule(None)
    res.run()
    _check_result(res, order, oracle, "plain again")
    res.close()
    ss.close()
    tbl.close()


def test_contig_ranges_and_chunks(ctx, monkeypatch):
    """the same contigs through pg_anchor_run_range over every contig subrange of a rows-only result (and over the ranges of a
    schedule by ranges), and through PG_RUN_CHUNKS = 2 and 3 with chunks of a few tiles: outputs equal the single launch's"""
    from panagram_amd import engine
    n, k = 3, 21
    genomes, dbs, anchors, oracle = _edge_case(n, k)
    tbl = _table(ctx, genomes, k, n, 15)
    nc = len(NKMERS)
    order = [(g, ci) for g in anchors for ci in range(nc)]
    ss1 = engine.SeqSet.from_host(ctx, genomes[1])
    whole = engine.AnchorResult(tbl, ss1, rows_only=True)
    whole.run()
    ctx.synchronize()
    want = [whole.download(ci, want_bitmap100=False)[0] for ci in range(nc)]
    for ci in range(nc):
        if (1, ci) in oracle:
            assert np.array_equal(want[ci], oracle[(1, ci)][0]), ci
    for c0 in range(nc):
        for c1 in range(c0 + 1, nc + 1):
            piece = engine.AnchorResult(tbl, ss1, rows_only=True)
            piece.run_range(c0, c1 - c0)
            ctx.synchronize()
            for ci in range(c0, c1):
                assert np.array_equal(piece.download(ci, want_bitmap100=False)[0], want[ci]), (c0, c1, ci)
            piece.close()
    whole.close()
    ss1.close()
    # a schedule by ranges: genome 0 alone, the other two side by side; whole ranges follow the schedule, others tile order
    ss = engine.SeqSet.from_host(ctx, [genomes[g][ci] for g, ci in order])
    group = np.repeat(np.arange(len(anchors), dtype=np.uint32), nc)
    res = engine.AnchorResult(tbl, ss, rows_only=True)
    res.coschedule_ranges(group, [0, nc], piece_tiles=3)
    for c0, cn in [(nc, 2 * nc), (0, nc), (nc + 3, 4), (0, 3 * nc)]:
        res.run_range(c0, cn)
    ctx.synchronize()
    _check_result(res, order, oracle, "ranges", stats=False)
    res.close()
    monkeypatch.setenv("PG_CHUNK_MIN_TILES", "4")
    for chunks in (2, 3):
        monkeypatch.setenv("PG_RUN_CHUNKS", str(chunks))
        res = engine.AnchorResult(tbl, ss)  # (plain order: the chunks are cut at the first run)
        res.run()
        _check_result(res, order, oracle, f"{chunks} chunks, plain")
        res.close()
        res = engine.AnchorResult(tbl, ss)
        res.coschedule(group, piece_tiles=3)  # (the chunks are slices of the schedule)
        res.run()
        _check_result(res, order, oracle, f"{chunks} chunks, co-scheduled")
        res.close()
    monkeypatch.delenv("PG_RUN_CHUNKS")
    monkeypatch.delenv("PG_CHUNK_MIN_TILES")
    ss.close()
    tbl.close()


@functools.lru_cache(maxsize=None)
def _repeat_family(k):
    """test_repeat_family_heavy_minimizer_groups' generator: 500 diverged copies of a 400-base element per genome, three
    genomes, ONE contig each — stretches of thousands of positions lie inside the family"""
    rng = np.random.default_rng(k)
    n = 3
    elem = rng.integers(0, 4, 400, dtype=np.uint8)
    genomes = []
    for g in range(n):
        parts = []
        for c in range(500):
            e = elem.copy()
            mut = rng.random(len(e)) < 0.04
            e[mut] = (e[mut] + rng.integers(1, 4, int(mut.sum()), dtype=np.uint8)) % 4
            parts += [e, rng.integers(0, 4, 30, dtype=np.uint8)]
        genomes.append([po.codes_to_ascii(np.concatenate(parts))])
    dbs = po.build_bitvec_dbs(genomes, k)
    o_rows, o_rows100, o_bins, _, o_cs = po.anchor_contig(dbs, genomes[1][0], k, n)
    return genomes, o_rows, o_rows100, o_bins, o_cs


@pytest.mark.parametrize("k,m", [(21, None), (31, 25)])
def test_queue_fills_in_a_repeat_family(ctx, k, m):
    """inside the family most keys sit outside their home lines: a tile meets more overflow entries than its queue may hold
    when a batch starts — the early drain in mid-tile, the batch loop's re-entry — and chains longer than the group's own
    lines (the lane chase, the key's own sequence).  k = 31 with m-mers of 25 bases: the M64 instantiation; every level's line
    is derived from the entry's group.  Rows of genome 1 before and after a rehash to four keys per line."""
    genomes, o_rows, o_rows100, o_bins, o_cs = _repeat_family(k)
    n = 3
    tbl = _table(ctx, genomes, k, n, m)
    if m is not None:
        assert tbl.minimizer == m > 16
    for dense in (False, True):
        if dense:
            tbl.rehash(4.0)
        rows, rows100, bins, cs = tbl.anchor_contig(genomes[1][0])
        assert np.array_equal(rows, o_rows), dense
        assert np.array_equal(rows100, o_rows100), dense
        assert np.array_equal(bins.astype(np.int64), o_bins) and np.array_equal(cs.astype(np.int64), o_cs), dense
    tbl.close()
