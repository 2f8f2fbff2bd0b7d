"""GPU: engine.NovelTable (k_novel_count, k_novel_grow, k_novel_scan) — a sample streamed through the pan table, its missing windows
counted in a key table that starts at 16 keys and grows in front of every add — against the numpy model (tests/novel_ref.py),
exactly: the sorted (key, depth) pairs, the counts at several thresholds from one table, every front end of the pan table's
placement (k), every layout of its lines, a sparse and a dense pan table, growth with the depths kept, the capacity protocol, the two
limits an add holds before it launches, and a stale handle's refusal.

At k = 6 the kernels are held to the model exactly as at every k, but the crafted sample's own exact promises — depth 2 for the key
spelled once per strand, the ``edge`` key at min_count - 1 and then min_count, the single depths of ``broken``, ``lower`` and
``exact`` — are asserted (tests/test_novel_cpu.py) from k = 21 on only (``novel_ref.EXACT_FROM_K``): among 2080 canonical 6-mers a
chance collision deepens them."""
import numpy as np
import pytest

from tests import novel_ref as NR

pytestmark = pytest.mark.gpu

K, MIN_COUNT, WIDTHS = NR.GPU_K, NR.GPU_MIN_COUNT, NR.GPU_WIDTHS
masks, load, pan_table = NR.masks, NR.load, NR.pan_table


_MODELS = {}


def model(k):
    """per k, computed once and left alone: (table keys, the sample's two sets, promises, the model after the first set, after both)"""
    if k not in _MODELS:
        table, sets, _, promises = NR.crafted(k, MIN_COUNT)
        _MODELS[k] = (table, sets, promises, NR.novel_counts(table, sets[:1], k), NR.novel_counts(table, sets, k))
    return _MODELS[k]


def same_result(got, ref, tag):
    assert sorted(got) == ["depth_hist", "nkeys", "solid", "solid_windows"], tag
    assert got["depth_hist"].dtype == np.int64 and got["depth_hist"].tolist() == ref["depth_hist"].tolist(), (tag, got["depth_hist"], ref["depth_hist"])
    for f in ("nkeys", "solid", "solid_windows"):
        assert got[f] == ref[f], (tag, f, got[f], ref[f])


def same_keys(got, nk, d, min_count, tag):
    """the sorted (key, depth) pairs, not only their histogram"""
    keys, depths = got
    wk, wd = NR.solid_keys(nk, d, min_count)
    assert keys.dtype == np.uint64 and depths.dtype == np.uint32 and len(keys) == len(wk), (tag, len(keys), len(wk))
    bad = np.flatnonzero((keys != wk) | (depths.astype(np.int64) != wd))
    assert len(bad) == 0, (tag, len(bad), keys[bad[:6]].tolist(), depths[bad[:6]].tolist(), wk[bad[:6]].tolist(), wd[bad[:6]].tolist())


def run_crafted(ctx, tbl, k, tag):
    """the crafted sample of ``k`` against ``tbl`` (which holds model(k)'s table keys), from a novel table created for 16 keys"""
    from panagram_amd import engine
    table, sets, p, first, both = model(k)
    pan_before = tbl.stats()
    nt = engine.NovelTable(tbl, capacity_keys=16)
    try:
        assert nt.stats() == {"nkeys": 0, "nslots": 32, "grown": 0}
        same_result(nt.result(1), NR.result([], 1), (tag, "untouched"))
        ssa, ssb = (engine.SeqSet.from_host(ctx, s) for s in sets)
        try:
            assert nt.add(ssa) == (first[0], first[1], len(first[2])), (tag, "windows, hits and new keys of the first set")
            st = nt.stats()
            assert st["grown"] == 1 and st["nkeys"] == len(first[2]) and st["nslots"] >= 2 * st["nkeys"], (tag, st)  # (an empty table grown)
            same_result(nt.result(MIN_COUNT), NR.result(first[3], MIN_COUNT), (tag, "first set"))
            same_keys(nt.keys(1), first[2], first[3], 1, (tag, "first set"))
            assert nt.add(ssb) == (both[0] - first[0], both[1] - first[1], len(both[2]) - len(first[2])), (tag, "the second set")
            t = engine.novel_last_timing()
            assert sorted(t) == ["count_ms", "grow_ms", "runs_ms", "scan_ms"] and t["count_ms"] > 0 and t["grow_ms"] > 0 and t["scan_ms"] > 0
        finally:
            ssa.close()
            ssb.close()
        st = nt.stats()
        assert st["grown"] >= 2 and st["nkeys"] == len(both[2]) and st["nslots"] >= 2 * st["nkeys"], (tag, st)  # (a table with keys grown)
        # the depths came through the growth: what the first set alone holds reads as before, the rest only went up
        keys, depths = nt.keys(1)
        at = np.searchsorted(keys, first[2])
        assert (keys[at] == first[2]).all() and (depths[at] >= first[3]).all()
        only_first = ~np.isin(first[2], NR.novel_counts(table, sets[1:], k)[2])
        assert only_first.sum() >= (300 if k >= 16 else 3) and (depths[at][only_first] == first[3][only_first]).all()
        for mc in (1, 2, 3, 300):
            same_result(nt.result(mc), NR.result(both[3], mc), (tag, "both sets, min_count", mc))
            same_keys(nt.keys(mc), both[2], both[3], mc, (tag, "both sets, min_count", mc))
        assert engine.novel_last_timing()["scan_ms"] > 0
        got = dict(zip(*(x.tolist() for x in nt.keys(300))))
        assert got[p["homo"]] == 300 and all(x in got for x in p["sat11"])  # (one counter for 64 lanes; past what a byte holds)
        # the capacity protocol: the first `cap` in slot order, the full number always; the same on every call
        k10, d10, n = nt.keys(2, cap=10)
        full = dict(zip(*(x.tolist() for x in nt.keys(2))))
        assert n == len(full) > 10 and len(k10) == 10 and len(set(k10.tolist())) == 10 and all(full[x] == y for x, y in zip(k10.tolist(), d10.tolist()))
        again = nt.keys(2, cap=10)
        assert again[0].tolist() == k10.tolist() and again[1].tolist() == d10.tolist() and again[2] == n
        assert nt.keys(2, cap=0)[2] == n and nt.keys(2, cap=n + 5)[2] == n
        assert tbl.stats() == pan_before  # (the pan table is only read)
        nt.clear()
        assert nt.stats()["nkeys"] == 0 and nt.stats()["nslots"] == st["nslots"]
        same_result(nt.result(1), NR.result([], 1), (tag, "cleared"))
        assert len(nt.keys(1)[0]) == 0
        ssa = engine.SeqSet.from_host(ctx, sets[0])
        try:
            assert nt.add(ssa) == (first[0], first[1], len(first[2]))
        finally:
            ssa.close()
        same_keys(nt.keys(1), first[2], first[3], 1, (tag, "the first set again"))
    finally:
        nt.close()


@pytest.mark.parametrize("n", WIDTHS)
def test_every_layout_of_the_pan_table(ctx, n):
    keys = model(K)[0]
    assert len(keys) >= 3000
    kw = dict(expected_keys=int(len(keys) * 1.02) + 64, keys_per_line=1.25) if n == 8 else {}
    tbl = pan_table(ctx, K, n, keys, **kw)
    try:
        if n == 8:
            st = tbl.stats()
            assert st["nslots"] // st["nbuckets"] == 14  # (14 keys to a line, a mask byte each)
        run_crafted(ctx, tbl, K, n)
    finally:
        tbl.close()


@pytest.mark.parametrize("k", [6, 31, 32])
def test_every_front_end_of_the_placement(ctx, k):
    """k = 6: the k-mer itself is hashed (no minimizer) and most canonical k-mers are in play; 31 and 32: 64-bit arithmetic, the
    keys next to the EMPTY mark"""
    tbl = pan_table(ctx, k, 8, model(k)[0])
    try:
        run_crafted(ctx, tbl, k, ("k", k))
    finally:
        tbl.close()


def test_a_sparse_and_a_dense_pan_table(ctx):
    keys = model(K)[0]
    tbl = pan_table(ctx, K, 33, keys, expected_keys=100 * len(keys))
    try:
        assert tbl.stats()["nslots"] > 100 * len(keys)
        run_crafted(ctx, tbl, K, "sparse")
    finally:
        tbl.close()
    tbl = pan_table(ctx, K, 33, keys)
    try:
        tbl.rehash(6.0)
        spilled, _ = tbl.spill()
        assert spilled > 0.02 and tbl.stats()["nslots"] < 2 * len(keys), (spilled, tbl.stats())
        run_crafted(ctx, tbl, K, "dense")
    finally:
        tbl.close()


def test_a_stale_pan_table_is_refused(ctx):
    """the keys were filtered by one geometry and key count of one table: a re-hash, an insert of new keys or a clear behind it"""
    from panagram_amd import engine
    keys, sets = model(K)[0], model(K)[1]
    M = masks(8, len(keys))
    tbl = engine.PanTable(ctx, K, 8)
    ss = engine.SeqSet.from_host(ctx, sets[0])
    try:
        load(tbl, keys[:-100], M[:-100])

        def refused(nt):
            for call in (lambda: nt.add(ss), lambda: nt.result(1), lambda: nt.keys(1)):
                with pytest.raises(engine.PanagramHipError) as ei:
                    call()
                assert ei.value.code == -1 and "changed behind the novel table" in str(ei.value)
            assert sorted(nt.stats()) == ["grown", "nkeys", "nslots"]
            nt.clear()  # (still the handle's own memory)
            nt.close()
        nt = engine.NovelTable(tbl, 16)
        nt.add(ss)
        tbl.rehash(6.0)
        refused(nt)
        nt = engine.NovelTable(tbl, 16)  # a new one answers
        w, h, new = nt.add(ss)
        ref = NR.novel_counts(keys[:-100], sets[:1], K)
        assert (w, h, new) == (ref[0], ref[1], len(ref[2]))
        same_keys(nt.keys(1), ref[2], ref[3], 1, "after the re-hash")
        load(tbl, keys[-100:], M[-100:])  # new keys
        refused(nt)
        nt = engine.NovelTable(tbl, 16)
        tbl.clear()
        refused(nt)
        nt = engine.NovelTable(tbl, 16)
        for bad in (0, 2 ** 32):
            with pytest.raises(ValueError, match="min_count"):
                nt.result(bad)
            with pytest.raises(ValueError, match="min_count"):
                nt.keys(bad)
        lib = ctx._lib
        assert lib.pg_novel_result(nt._h, 0, None, None, None, None) == -1 and b"min_count" in lib.pg_last_error()
        assert lib.pg_novel_result(nt._h, 1, None, None, None, None) == 0  # (every output may be NULL)
        assert lib.pg_novel_add_seqset(nt._h, None, None, None, None) == -1 and b"NULL" in lib.pg_last_error()
        assert lib.pg_novel_create(None, 16, None) == -1 and b"pg_novel_create" in lib.pg_last_error()
        for cap in (0, 2 ** 30 + 1):
            with pytest.raises(engine.PanagramHipError) as ei:
                engine.NovelTable(tbl, cap)
            assert ei.value.code == -1 and "capacity" in str(ei.value)
        nt.close()
        nt.close()
        nt = engine.NovelTable(tbl, 16)
        tbl.close()  # the table closes its novel tables first
        assert nt._h is None
    finally:
        ss.close()
        tbl.close()


def test_the_two_limits_of_an_add_are_held_before_anything_is_launched(ctx):
    """more than 2^30 keys and positions: PG_E_CAPACITY; more than 2^32 - 1 windows in a handle: PG_E_INVALID — both from the
    lengths alone (the sequence sets below are never read), and the handle answers as before afterwards"""
    from panagram_amd import engine
    keys, sets, _, first, _ = model(K)
    tbl = pan_table(ctx, K, 8, keys)
    nt = engine.NovelTable(tbl, 16)
    ss = engine.SeqSet.from_host(ctx, sets[0])
    try:
        assert nt.add(ss) == (first[0], first[1], len(first[2]))
        before = nt.stats()
        big = engine.SeqSet(ctx, [2 ** 30 + K])  # 2^30 + 1 positions
        try:
            with pytest.raises(engine.PanagramHipError) as ei:
                nt.add(big)
            assert ei.value.code == -4 and "batch-bytes" in str(ei.value)
        finally:
            big.close()
        huge = engine.SeqSet(ctx, [2 ** 32 + K - 1 - first[0]])  # the windows added so far and these positions: 2^32
        try:
            with pytest.raises(engine.PanagramHipError) as ei:
                nt.add(huge)
            assert ei.value.code == -1 and "2^32 - 1" in str(ei.value)
        finally:
            huge.close()
        assert nt.stats() == before
        same_keys(nt.keys(1), first[2], first[3], 1, "after the two refusals")
        assert nt.add(ss)[:2] == (first[0], first[1])  # (usable)
        same_keys(nt.keys(1), first[2], 2 * first[3], 1, "the first set twice")
    finally:
        ss.close()
        nt.close()
        tbl.close()


def test_an_empty_pan_table_and_an_empty_sequence_set(ctx):
    from panagram_amd import engine
    keys, sets = model(K)[0], model(K)[1]
    tbl = engine.PanTable(ctx, K, 5)
    try:
        nt = engine.NovelTable(tbl, 16)
        ss = engine.SeqSet.from_host(ctx, sets[0])
        ref = NR.novel_counts(np.zeros(0, np.uint64), sets[:1], K)
        try:
            assert nt.add(ss) == (ref[0], 0, len(ref[2]))  # every window is novel
        finally:
            ss.close()
        same_keys(nt.keys(1), ref[2], ref[3], 1, "an empty pan table")
        nt.close()
    finally:
        tbl.close()
    tbl = pan_table(ctx, K, 8, keys)
    try:
        nt = engine.NovelTable(tbl, 16)
        empty, nreads, used = engine.SeqSet.from_fastq(ctx, b"")  # one contig of no base
        short = engine.SeqSet.from_host(ctx, [b"ACGT", b"N" * 30, b"ACGTACGTACGTACGTACGT"])  # no contig holds a window
        try:
            assert (nreads, used) == (0, 0) and nt.add(empty) == (0, 0, 0) and nt.add(short) == (0, 0, 0)
        finally:
            empty.close()
            short.close()
        assert nt.stats() == {"nkeys": 0, "nslots": 32, "grown": 0}
        same_result(nt.result(1), NR.result([], 1), "nothing added")
        nt.close()
    finally:
        tbl.close()
