"""GPU: the byte-mask table layout (pg_device.h LAYOUT_BYTEMASK: tables of up to 8 genomes created through pg_table_create_dense —
a 128-byte line of two halves of seven bare keys and seven mask bytes, a key in the half its parity names) against the oracle:
rows of every front end (direct mode, 32-bit and 64-bit m-mers), co-scheduled and genome by genome; the edges of the rule that
chooses the layout; full halves (overflow queue, early drain, staged level, lane chase); the mask bytes; every table operation;
the sharded mode's bit columns; and the premise — at most half the keys outside their home half-line."""
import os
import tempfile

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import kmerstats_ref as KR

pytestmark = pytest.mark.gpu

KPL = 1.25  # keys per 128-byte line the flagship's table is created for


def _ascii(gen):
    return [[po.codes_to_ascii(c) for c in g] for g in gen]


def _with_extras(genomes, seed):
    """a run of N in the first genome's first contig (the masked path), a contig shorter than a tile, and poly-A / poly-T
    stretches (AA..A and TT..T are one canonical k-mer, 0: next to the EMPTY and TOMB key values at k = 32)"""
    rng = np.random.default_rng(seed)
    c0 = bytearray(genomes[0][0])
    c0[5000:5045] = b"N" * 45
    c0[9000] = ord("N")
    genomes[0][0] = bytes(c0)
    short = po.codes_to_ascii(rng.integers(0, 4, 300, dtype=np.uint8))
    poly = b"A" * 90 + short[:40] + b"T" * 90 + b"TG" + b"T" * 40
    for g in range(len(genomes)):
        genomes[g] = list(genomes[g]) + [short if g % 2 == 0 else short[::-1], poly]
    return genomes


_CASES = {}


def case(n, k):
    """(genomes, dbs) per (genome count, k), computed once and left alone"""
    if (n, k) not in _CASES:
        genomes = _with_extras(_ascii(po.synth_genomes(n, [30_000, 2_500], 0.02, 100 * n + k)), n + k)
        _CASES[(n, k)] = (genomes, po.build_bitvec_dbs(genomes, k))
    return _CASES[(n, k)]


def build(ctx, genomes, k, n=None, kpl=KPL, dense=True, nkeys=None):
    from panagram_amd import engine
    n = n or len(genomes)
    if nkeys is None:
        nkeys = len(po.build_bitvec_dbs(genomes, k)[0][0])
    tbl = engine.PanTable(ctx, k, n, expected_keys=int(nkeys * 1.02) + 64, **({"keys_per_line": kpl} if dense else {}))
    for g, contigs in enumerate(genomes):
        ss = engine.SeqSet.from_host(ctx, contigs)
        tbl.insert_seqset(g, ss)
        ss.close()
    return tbl


def slots_per_line(tbl):
    st = tbl.stats()
    return st["nslots"] // st["nbuckets"]


def check_rows(ctx, tbl, genomes, dbs, k, n, which=None):
    """genome by genome (one launch per contig) and co-scheduled (one launch over every genome's contigs)"""
    from panagram_amd import engine
    which = range(len(genomes)) if which is None else which
    oracle = {(g, i): po.anchor_contig(dbs, seq, k, n)[0] for g in which for i, seq in enumerate(genomes[g])}
    for g in which:
        for i, seq in enumerate(genomes[g]):
            assert np.array_equal(tbl.anchor_contig(seq)[0], oracle[(g, i)]), ("per genome", g, i)
    sets = [engine.SeqSet.from_host(ctx, genomes[g]) for g in which]
    both = engine.SeqSet.concat(ctx, sets)
    res = engine.AnchorResult(tbl, both, colsums=True)
    groups = [gi for gi, g in enumerate(which) for _ in genomes[g]]
    res.coschedule(groups, 2)
    res.run()
    ci = 0
    for g in which:
        for i in range(len(genomes[g])):
            assert np.array_equal(res.download(ci)[0], oracle[(g, i)]), ("co-scheduled", g, i)
            ci += 1
    for x in (res, both, *sets):
        x.close()


@pytest.mark.parametrize("k", [12, 20, 21, 27, 31, 32])
@pytest.mark.parametrize("n", [1, 2, 7, 8])
def test_rows_equal_the_oracle(ctx, n, k):
    genomes, dbs = case(n, k)
    tbl = build(ctx, genomes, k, nkeys=len(dbs[0][0]))
    try:
        assert slots_per_line(tbl) == 14
        assert (tbl.minimizer > 16) == (k >= 27) and (tbl.minimizer == 0) == (k < 20)
        assert tbl.stats()["nkeys"] == len(dbs[0][0])
        check_rows(ctx, tbl, genomes, dbs, k, n, which=sorted({0, n - 1}))
    finally:
        tbl.close()


def test_edges_of_the_rule(ctx, monkeypatch):
    """8 genomes take the new lines through pg_table_create_dense and 9 the old; plain pg_table_create and PG_BYTEMASK_LAYOUT=0
    keep 8 slots; the rows are the oracle's in every case"""
    k = 21
    genomes9 = _ascii(po.synth_genomes(9, [20_000, 1_500], 0.02, 99))
    for n, dense, env, want in [(8, True, None, 14), (9, True, None, 8), (8, False, None, 8), (8, True, "0", 8), (8, True, "1", 14)]:
        if env is None:
            monkeypatch.delenv("PG_BYTEMASK_LAYOUT", raising=False)
        else:
            monkeypatch.setenv("PG_BYTEMASK_LAYOUT", env)
        genomes = genomes9[:n]
        dbs = po.build_bitvec_dbs(genomes, k)
        tbl = build(ctx, genomes, k, dense=dense, nkeys=len(dbs[0][0]))
        try:
            assert slots_per_line(tbl) == want, (n, dense, env)
            check_rows(ctx, tbl, genomes, dbs, k, n, which=[0, n - 1])
        finally:
            tbl.close()


def _tandem_genomes(n, seed):
    """a tandem repeat of a 57-base unit, every copy with its own SNPs (3 %): thousands of distinct k-mers behind a handful of
    minimizers; a stretch of EXACT copies (one k-mer many times inside one tile); a tandem of 18-base units A x 15 + three bases
    that vary from copy to copy and genome to genome — the canonical 15-mer of A x 15 is 0, the smallest rank there is, so at
    k = 21 (m = 15) 7 of every 18 positions (the windows that hold a whole A x 15) belong to ONE group of thousands of distinct
    keys: about 400 of a tile's 1024 positions overflow, more than the 256 its queue takes before the early drain, and go on
    through the staged level and the lane-by-lane chase; unique sequence around"""
    rng = np.random.default_rng(seed)
    unit = rng.integers(0, 4, 57, dtype=np.uint8)
    out = []
    for g in range(n):
        copies = np.tile(unit, 120)
        snp = rng.random(len(copies)) < 0.03
        copies[snp] = (copies[snp] + rng.integers(1, 4, int(snp.sum()), dtype=np.uint8)) % 4
        core = np.zeros((400, 18), np.uint8)
        core[:, 15:] = rng.integers(0, 4, (400, 3), dtype=np.uint8)
        flank = [rng.integers(0, 4, 3_000, dtype=np.uint8) for _ in range(2)]
        out.append([po.codes_to_ascii(np.concatenate([flank[0], copies, np.tile(unit, 40), core.ravel(), flank[1]]))])
    return out


@pytest.mark.parametrize("what", ["tandem", "six_per_line"])
def test_full_halves(ctx, what):
    k = 21
    if what == "tandem":
        genomes, kpl = _tandem_genomes(8, 5), KPL
    else:
        genomes, kpl = case(8, 21)[0], 6.0
    dbs = po.build_bitvec_dbs(genomes, k)
    tbl = build(ctx, genomes, k, kpl=kpl, nkeys=len(dbs[0][0]))
    try:
        assert slots_per_line(tbl) == 14 and tbl.stats()["nkeys"] == len(dbs[0][0])
        spill = tbl.measure_spill()
        assert spill > 0
        if what == "tandem":
            # the premise of _tandem_genomes: the table's minimizers are 15-mers, and the windows that hold a whole A x 15 form
            # ONE group.  Its distinct keys: the 7 window offsets hold 3, 3, 4, 5, 6, 5 and 4 varying bases, drawn 8 x 400 times
            # each — 64 + 64 + 256 + 979 + 2221 + 979 + 256 = 4819 expected distinct keys (V (1 - exp(-3200 / V)) of V = 4^bases
            # variants), of which 14 fit the home line: more than 4000 keys outside it whatever the draw (and the SNP tandem's
            # on top).  Should the minimizer order change and A x 15 stop being the smallest m-mer, this falls to a few hundred.
            assert tbl.minimizer == 15
            print("tandem: keys outside their home line", round(spill * len(dbs[0][0])), "of", len(dbs[0][0]))
            assert spill * len(dbs[0][0]) > 4000, (spill, len(dbs[0][0]))
        check_rows(ctx, tbl, genomes, dbs, k, 8, which=[0, 7])
    finally:
        tbl.close()


def test_mask_bytes(ctx):
    """neighbouring slots of a half get their bytes from different genomes in different launches; a k-mer of all 8 genomes reads
    0xFF; poly-A / poly-T k-mers at k = 32 (canonical value 0) are keys like any other"""
    k, n = 32, 8
    genomes, dbs = case(n, k)
    tbl = build(ctx, genomes, k, nkeys=len(dbs[0][0]))
    try:
        keys, vals = tbl.export(0)
        o = np.argsort(keys)
        assert np.array_equal(keys[o], dbs[0][0]) and np.array_equal(vals[o], dbs[0][1])
        assert keys.min() == 0 and (vals == 0xFF).any() and len(np.unique(vals)) > 20
        poly = genomes[0][-1]
        rows = tbl.anchor_contig(poly)[0]
        assert np.array_equal(rows, po.anchor_contig(dbs, poly, k, n)[0]) and rows[0, 0] == 0xFF
        assert np.array_equal(tbl.counters_for_read(0, genomes[3][0][:3000]), po.counters_for_read(dbs[0], genomes[3][0][:3000], k))
    finally:
        tbl.close()


def _mask_matrix(masks, n):
    return ((masks[:, None] >> np.arange(n, dtype=np.uint32)[None, :]) & 1).astype(np.uint8)


def test_table_operations(ctx):
    from panagram_amd import engine
    k, n = 21, 8
    genomes = _tandem_genomes(n, 11)
    dbs = po.build_bitvec_dbs(genomes, k)
    nkeys = len(dbs[0][0])
    ref = KR.stats(dbs[0][0], _mask_matrix(dbs[0][1], n))
    tbl = build(ctx, genomes, k, kpl=3.0, nkeys=nkeys)
    try:
        def same_table(tag):
            assert slots_per_line(tbl) == 14 and tbl.stats()["nkeys"] == nkeys, tag
            keys, vals = tbl.export(0)
            o = np.argsort(keys)
            assert np.array_equal(keys[o], dbs[0][0]) and np.array_equal(vals[o], dbs[0][1]), tag
            got = tbl.kmer_stats()
            assert got["nkeys"] == nkeys and np.array_equal(got["pairs"], ref["pairs"]), tag
            assert got["occupancy"].tolist() == ref["occupancy"].tolist() and got["private"].tolist() == ref["private"].tolist(), tag
        same_table("built")  # (the exact copies: one k-mer many times inside one tile takes one slot)
        assert 0.0 < tbl.measure_spill() < 1.0
        tbl.rehash(6.0)
        same_table("dense")
        assert tbl.spill()[0] > 0 and tbl.spill()[1] == 14
        tbl.rehash(1.5)
        same_table("sparse again")
        # clear, and the anchors' table of genome 0 updated with the others' bits: the keys of genome 0, the masks of all
        tbl.clear()
        assert tbl.stats()["nkeys"] == 0 and len(tbl.export(0)[0]) == 0 and tbl.kmer_stats()["nkeys"] == 0
        sets = [engine.SeqSet.from_host(ctx, g) for g in genomes]
        tbl.insert_seqset(0, sets[0])
        for g in range(1, n):
            tbl.update_seqset(g, sets[g])
        own = (dbs[0][1] & 1) != 0
        keys, vals = tbl.export(0)
        o = np.argsort(keys)
        assert tbl.stats()["nkeys"] == int(own.sum())
        assert np.array_equal(keys[o], dbs[0][0][own]) and np.array_equal(vals[o], dbs[0][1][own])
        # ... and a rebuild in the same allocation
        bytes0 = tbl.stats()["bytes"]
        tbl.clear()
        for g in range(n):
            tbl.insert_seqset(g, sets[g])
        assert tbl.stats()["bytes"] == bytes0
        same_table("rebuilt")
        check_rows(ctx, tbl, genomes, dbs, k, n, which=[2])
        for s in sets:
            s.close()
    finally:
        tbl.close()
    # KMC import into such a table: the records' counters are the masks
    with tempfile.TemporaryDirectory() as d:
        po.write_kmc1(os.path.join(d, "db"), dbs[0][0], dbs[0][1], k)
        t2 = engine.PanTable(ctx, k, n, expected_keys=nkeys, keys_per_line=KPL)
        try:
            t2.load_kmc_files(0, os.path.join(d, "db"))
            assert slots_per_line(t2) == 14 and t2.stats()["nkeys"] == nkeys
            keys, vals = t2.export(0)
            o = np.argsort(keys)
            assert np.array_equal(keys[o], dbs[0][0]) and np.array_equal(vals[o], dbs[0][1])
            assert np.array_equal(t2.anchor_contig(genomes[5][0])[0], po.anchor_contig(dbs, genomes[5][0], k, n)[0])
        finally:
            t2.close()


@pytest.mark.parametrize("block", [(3, 4), (5, 7)])
def test_columns_of_one_and_two_genome_blocks(ctx, block):
    """the sharded planner's block tables: the probe's bit columns (ROWMODE 3) equal the bits of its rows"""
    import torch
    from panagram_amd import engine
    k = 21
    g_lo, g_hi = block
    width = g_hi - g_lo
    genomes, _ = case(8, k)
    mine = genomes[g_lo:g_hi]
    tbl = build(ctx, mine, k)
    try:
        assert slots_per_line(tbl) == 14
        sets = [engine.SeqSet.from_host(ctx, genomes[g][:2]) for g in (0, 3, 7)]
        merged = engine.SeqSet.concat_ranges(ctx, [(s_, 0, 1) for s_ in sets] + [(s_, 1, 1) for s_ in sets])
        rows = engine.AnchorResult(tbl, merged, colsums=False, rows_only=True)
        cols = engine.AnchorResult(tbl, merged, colsums=False, columns_only=True)
        assert cols.columns_direct(width)
        for r_ in (rows, cols):
            r_.coschedule_ranges([0, 1, 2, 0, 1, 2], [0, 3], 2)
        dbs = po.build_bitvec_dbs(mine, k)
        for c0, nc in [(0, 3), (3, 3)]:
            nb_ = rows.columns_bytes_range(width, c0, nc)
            a = torch.zeros(nb_, dtype=torch.uint8, device="cuda")
            b = torch.full((nb_,), 0xAB, dtype=torch.uint8, device="cuda")
            rows.run_range(c0, nc)
            rows.extract_columns_range(0, width, c0, nc, a.data_ptr())
            cols.run_columns_range(c0, nc, width, b.data_ptr())
            ctx.synchronize()
            assert a.any() and torch.equal(a, b)
        for ci, g in enumerate((0, 3, 7)):  # (and the rows themselves are the oracle's)
            assert np.array_equal(rows.download(ci, want_bitmap100=False)[0], po.anchor_contig(dbs, genomes[g][0], k, width)[0])
        for x in (rows, cols, merged, *sets):
            x.close()
    finally:
        tbl.close()


@pytest.mark.parametrize("per,kpl", [(2, 4.5), (1, 3.5)])
def test_sharded_passes_take_columns_straight_from_the_probe(ctx, monkeypatch, per, kpl):
    """the product's sharded path (ShardedAnchoring through bench.config5_leg, at a hundredth of configs[4]'s length): a DENSE
    block table of one or two genomes has byte-mask lines, and its passes still take the bit columns from the probe itself —
    no narrow row buffer, no extract — with rows equal to the oracle's heads and tails"""
    import types
    import torch
    import bench
    from panagram_amd import distributed as pdist
    from panagram_amd import engine
    monkeypatch.delenv("PG_BYTEMASK_LAYOUT", raising=False)
    monkeypatch.setattr(engine, "COLUMNS_DIRECT", True)
    monkeypatch.setattr(pdist.ShardedAnchoring, "DIRECT_MAX_WIDTH", 2)
    probe = engine.PanTable(ctx, 21, per, expected_keys=1_000_000, keys_per_line=kpl)
    assert slots_per_line(probe) == 14
    probe.close()
    dev = torch.device("cuda", 0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        out = bench.config5_leg(ctx, dev, types.SimpleNamespace(seed=4321), genome_mb=30, contigs=6, sample_n=100_000, per=per, keys_per_line=kpl)
    finally:
        ctx.set_stream(None)
    assert out["columns_straight_from_the_probe"] is True
    assert out["rows_equal_gpu"] is True, out["rows_check"]
    assert out["anchors_hold_all_own_kmers"] and out["anchors_completed"] == 8 and out["genomes_per_block"] == per


def test_premise_half_the_spill(ctx, monkeypatch):
    """8 x 2 Mb, d = 1 %, k = 21, 1.25 keys per line: the byte-mask table leaves at most half as many keys outside their home
    (half-)line as the 8-slot table of the same bytes (tools/spill_model.py says a quarter)"""
    from panagram_amd import engine
    k, n = 21, 8
    genomes = _ascii(po.synth_genomes(n, [2_000_000], 0.01, 4242))
    sets = [engine.SeqSet.from_host(ctx, g) for g in genomes]
    spill, nkeys = {}, None
    for env in ("0", "1"):
        monkeypatch.setenv("PG_BYTEMASK_LAYOUT", env)
        if nkeys is None:  # the distinct k-mers, counted by a table of the library's own density
            t0 = engine.PanTable(ctx, k, n)
            for g in range(n):
                t0.insert_seqset(g, sets[g])
            nkeys = t0.stats()["nkeys"]
            t0.close()
        tbl = engine.PanTable(ctx, k, n, expected_keys=nkeys, coscheduled=n, keys_per_line=KPL)
        for g in range(n):
            tbl.insert_seqset(g, sets[g])
        assert tbl.stats()["nkeys"] == nkeys and slots_per_line(tbl) == (8 if env == "0" else 14)
        assert abs(nkeys / tbl.stats()["nbuckets"] - KPL) < 0.05
        spill[env] = tbl.measure_spill()
        tbl.close()
    for s in sets:
        s.close()
    print("keys outside their home line: 8 slots", spill["0"], "byte-mask", spill["1"])
    assert 0 < spill["1"] <= 0.5 * spill["0"], spill
