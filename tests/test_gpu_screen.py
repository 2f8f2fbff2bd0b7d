"""GPU: engine.TableScreen (k_table_mark, k_table_screen) — a sample streamed through the pan table and the counts of one pass over
its slots, against the numpy model (tests/screen_ref.py), exactly: crafted masks at every layout and mask width, every front end of
the table's placement (k), sparse and dense tables, saturation without a carry into a neighbouring byte, tables built from
sequence (retired slots among them), accumulation over calls, one plane read at several thresholds, and a stale handle's refusal."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import copies_ref as CR
from tests import kmerstats_ref as KR
from tests import screen_ref as SR

pytestmark = pytest.mark.gpu

K = 21
NKEYS = 3000
MIN_COUNT = 2  # what the crafted sample's two special depths straddle
# every layout and every word count that changes a path: slots (W = 1: 1, 8, 32; W = 2: 33, 64), inline (W = 3: 65, 96), split
# (W = 4: 97; 5: 129; 16: 512, the widest)
WIDTHS = [1, 8, 32, 33, 64, 65, 96, 97, 129, 512]
FIELDS = ("distinct", "seen", "private", "private_seen", "occ", "seen_occ", "depth_hist", "core_depth_hist")


def masks(n, nkeys, seed=0):
    """M: all-ones keys, one key private to every genome, keys whose only bits lie in the last 32-genome word, random masks of
    every density for the rest; no key without a bit.  The rows are dealt to the keys at random: the table's special keys and the
    sample's (the first of ``SR.table_keys``) get whatever falls to them"""
    rng = np.random.default_rng(1000 * n + seed)
    M = (rng.random((nkeys, n)) < rng.random((nkeys, 1))).astype(np.uint8)
    M[:10] = 1
    M[10:10 + min(n, nkeys - 40)] = np.eye(n, dtype=np.uint8)[:min(n, nkeys - 40)]
    last0 = 32 * ((n - 1) // 32)
    tail = M[nkeys - 20:]
    tail[:, :last0] = 0
    tail[:, n - 1] |= (tail[:, last0:].sum(axis=1) == 0).astype(np.uint8)
    none = M.sum(axis=1) == 0
    M[none, rng.integers(0, n, int(none.sum()))] = 1
    return M[rng.permutation(nkeys)]


def load(tbl, keys, M):
    """through PanTable.insert_keys: one call per 32-genome group, with the keys whose word is non-zero there"""
    for d, words in enumerate(KR.group_words(M)):
        has = words != 0
        tbl.insert_keys(d, keys[has], words[has])


def same(got, ref, tag):
    for f in FIELDS:
        assert got[f].dtype == np.int64 and got[f].shape == ref[f].shape, (tag, f)
        bad = np.flatnonzero(got[f] != ref[f])
        assert len(bad) == 0, (tag, f, len(bad), bad[:6].tolist(), got[f][bad[:6]].tolist(), ref[f][bad[:6]].tolist())
    assert got["nkeys"] == ref["nkeys"], (tag, "nkeys", got["nkeys"], ref["nkeys"])


_SAMPLES = {}


def sample(k):
    """per k, computed once and left alone: (keys, the crafted sample's two sets, its promises, (windows, hits, depths) after the
    first set, the same after both)"""
    if k not in _SAMPLES:
        keys = SR.table_keys(np.random.default_rng(k), NKEYS, k)
        sets, promises = SR.crafted_sample(keys, k, MIN_COUNT, np.random.default_rng(100 + k))
        _SAMPLES[k] = (keys, sets, promises, SR.depths(keys, sets[:1], k), SR.depths(keys, sets, k))
    return _SAMPLES[k]


def run_crafted(ctx, tbl, k, M, tag):
    """the crafted sample of ``k`` through ``tbl`` (which holds sample(k)'s keys with ``M``): the first set, a result; the second
    set, results at four thresholds from the one plane; clear, a result"""
    from panagram_amd import engine
    keys, sets, promises, first, both = sample(k)
    sc = engine.TableScreen(tbl)
    try:
        same(sc.result(1), SR.screen(keys, M, np.zeros(len(keys), np.int64), 1), (tag, "untouched"))
        ssa, ssb = (engine.SeqSet.from_host(ctx, s) for s in sets)
        try:
            assert sc.add(ssa) == (first[0], first[1]), (tag, "windows and hits of the first set")
            same(sc.result(MIN_COUNT), SR.screen(keys, M, first[2], MIN_COUNT), (tag, "first set"))
            assert sc.add(ssb) == (both[0] - first[0], both[1] - first[1]), (tag, "windows and hits of the second set")
        finally:
            ssa.close()
            ssb.close()
        at = keys.tolist().index(promises["at"])
        assert first[2][at] == MIN_COUNT - 1 and both[2][at] == MIN_COUNT  # (the second call makes it seen)
        for mc in (1, 2, 3, 255):
            same(sc.result(mc), SR.screen(keys, M, both[2], mc), (tag, "both sets, min_count", mc))
        t = engine.screen_last_timing()
        assert sorted(t) == ["mark_ms", "screen_ms"] and t["mark_ms"] > 0 and t["screen_ms"] > 0
        sc.clear()
        got = sc.result(1)
        assert not got["seen"].any() and not got["seen_occ"].any() and not got["private_seen"].any()
        assert got["depth_hist"][0] == got["nkeys"] == len(keys) and got["distinct"].tolist() == M.sum(axis=0).tolist()
    finally:
        sc.close()


@pytest.mark.parametrize("n", WIDTHS)
def test_crafted_masks_at_every_layout_and_width(ctx, n):
    from panagram_amd import engine
    keys = sample(K)[0]
    M = masks(n, NKEYS)
    ref = SR.screen(keys, M, sample(K)[4][2], 1)
    assert ref["occ"][n] >= 10 and (ref["private"] >= 1).all() and ref["occ"][0] == 0 and ref["seen"].max() > 100
    tbl = engine.PanTable(ctx, K, n)
    try:
        load(tbl, keys, M)
        assert tbl.stats()["nkeys"] == NKEYS
        run_crafted(ctx, tbl, K, M, n)
    finally:
        tbl.close()


def test_byte_mask_layout(ctx):
    """8 genomes in a table created for a known density: 14 keys to a line, a mask byte each"""
    from panagram_amd import engine
    keys = sample(K)[0]
    M = masks(8, NKEYS, seed=1)
    tbl = engine.PanTable(ctx, K, 8, expected_keys=int(NKEYS * 1.02) + 64, keys_per_line=1.25)
    try:
        load(tbl, keys, M)
        st = tbl.stats()
        assert st["nslots"] // st["nbuckets"] == 14 and st["nkeys"] == NKEYS
        run_crafted(ctx, tbl, K, M, "byte masks")
    finally:
        tbl.close()


@pytest.mark.parametrize("k", [15, 31, 32])
def test_every_front_end_of_the_placement(ctx, k):
    """k = 15: the k-mer itself is hashed (no minimizer); 31 and 32: 64-bit arithmetic, the keys next to the EMPTY and retired marks"""
    from panagram_amd import engine
    keys = sample(k)[0]
    M = masks(8, NKEYS, seed=k)
    tbl = engine.PanTable(ctx, k, 8)
    try:
        load(tbl, keys, M)
        assert (tbl.minimizer == 0) == (k == 15)
        run_crafted(ctx, tbl, k, M, ("k", k))
    finally:
        tbl.close()


@pytest.mark.parametrize("n", [8, 97])
def test_a_table_created_for_a_hundred_times_its_keys(ctx, n):
    """most chunks of the pass hold no key"""
    from panagram_amd import engine
    keys = sample(K)[0]
    M = masks(n, NKEYS, seed=2)
    tbl = engine.PanTable(ctx, K, n, expected_keys=100 * NKEYS)
    try:
        load(tbl, keys, M)
        assert tbl.stats()["nslots"] > 100 * NKEYS
        run_crafted(ctx, tbl, K, M, (n, "sparse"))
    finally:
        tbl.close()


DENSE_DEPTHS = (0, 1, 2, 3, 64, 254, 255, 300)


@pytest.fixture(scope="module")
def dense_case():
    """every key at a depth drawn from DENSE_DEPTHS: that many copies of its k bases on either strand, all copies of all keys
    shuffled and joined by N into one contig per set, two sets.  (keys, sets, depths by construction, model after the first set,
    model after both)"""
    rng = np.random.default_rng(77)
    keys = sample(K)[0]
    want = rng.choice(DENSE_DEPTHS, len(keys))
    want[:len(DENSE_DEPTHS)] = DENSE_DEPTHS  # (every depth occurs)
    which = rng.permutation(np.repeat(np.arange(len(keys)), want))
    spelled = [(SR.spell(int(x), K), SR.revcomp(SR.spell(int(x), K))) for x in keys]
    flip = rng.random(len(which)) < 0.5
    half = len(which) // 2
    sets = [[b"N".join(spelled[i][int(f)] for i, f in zip(which[a:b], flip[a:b]))] for a, b in ((0, half), (half, len(which)))]
    return keys, sets, want, SR.depths(keys, sets[:1], K), SR.depths(keys, sets, K)


@pytest.mark.parametrize("n", [8, 65, 129])
def test_saturation_in_a_dense_table_never_carries_into_a_neighbour(ctx, dense_case, n):
    """a table re-hashed so dense that groups spill past their home line and the four bytes of a dword are all live; depths up to
    300 through two calls.  The whole depth histogram is the model's: a carry out of one byte would move its neighbour's bin"""
    from panagram_amd import engine
    keys, sets, want, first, both = dense_case
    # the test's own premises: the depths are what was spelled, every junction window holds the N; a depth crosses 255 in the second call
    assert both[2].tolist() == np.minimum(want, SR.DEPTH_MAX).tolist() and both[0] == both[1] == int(want.sum())
    assert ((first[2] < SR.DEPTH_MAX) & (want == 300)).sum() > 100 and (first[2][want == 300] > 64).all()
    M = masks(n, NKEYS, seed=3)
    tbl = engine.PanTable(ctx, K, n)
    try:
        load(tbl, keys, M)
        tbl.rehash(6.0)
        spilled, _ = tbl.spill()
        assert spilled > 0.02 and tbl.stats()["nslots"] < 2 * NKEYS, (spilled, tbl.stats())
        sc = engine.TableScreen(tbl)
        try:
            ssa, ssb = (engine.SeqSet.from_host(ctx, s) for s in sets)
            try:
                assert sc.add(ssa) == (first[0], first[1])
                same(sc.result(1), SR.screen(keys, M, first[2], 1), (n, "dense, first call"))
                assert sc.add(ssb) == (both[0] - first[0], both[1] - first[1])
            finally:
                ssa.close()
                ssb.close()
            for mc in (1, 3, 255):
                got, ref = sc.result(mc), SR.screen(keys, M, both[2], mc)
                same(got, ref, (n, "dense, both calls", mc))
                assert got["depth_hist"].tolist() == ref["depth_hist"].tolist()
            hist = np.bincount(np.minimum(np.minimum(want, SR.DEPTH_MAX), 63), minlength=64)
            assert got["depth_hist"].tolist() == hist.tolist()
        finally:
            sc.close()
    finally:
        tbl.close()


def _repeat_genomes():
    """many diverged copies of one element: the build's racing claims leave retired slots behind"""
    rng = np.random.default_rng(1)
    elem = rng.integers(0, 4, 400, dtype=np.uint8)
    genomes = []
    for g in range(3):
        parts = []
        for c in range(300):
            e = elem.copy()
            mut = rng.random(len(e)) < 0.03
            e[mut] = (e[mut] + rng.integers(1, 4, int(mut.sum()), dtype=np.uint8)) % 4
            parts += [e, rng.integers(0, 4, 50, dtype=np.uint8)]
        genomes.append([po.codes_to_ascii(np.concatenate(parts))])
    return genomes


@pytest.mark.parametrize("kind", ["diverged", "repeats"])
def test_tables_built_from_sequence(ctx, kind):
    """insert_seqset for all genomes but the last, update_seqset for the last (its bit only where the table holds the k-mer
    already); each genome in turn as the sample recovers itself whole"""
    from panagram_amd import engine
    genomes = ([[po.codes_to_ascii(c) for c in g] for g in po.synth_genomes(5, [20000, 700], 0.02, 5)] if kind == "diverged"
               else _repeat_genomes())
    n = len(genomes)
    keys, M = KR.from_groups(po.build_bitvec_dbs(genomes[:-1], K), n - 1)
    last = np.isin(keys, np.unique(CR.valid_keys(genomes[-1], K))).astype(np.uint8)
    M = np.concatenate([M, last[:, None]], axis=1)
    tbl = engine.PanTable(ctx, K, n)
    try:
        sets = [engine.SeqSet.from_host(ctx, g) for g in genomes]
        for g in range(n - 1):
            tbl.insert_seqset(g, sets[g])
        tbl.update_seqset(n - 1, sets[n - 1])
        assert tbl.stats()["nkeys"] == len(keys)
        sc = engine.TableScreen(tbl)
        try:
            for g in range(n):
                ref, windows, hits = SR.screen_sets(keys, M, [genomes[g]], K, 1)
                assert sc.add(sets[g]) == (windows, hits), (kind, g)
                got = sc.result(1)
                same(got, ref, (kind, g))
                assert got["seen"][g] == got["distinct"][g] > 0
                if g < n - 1:
                    assert hits == windows and got["private_seen"][g] == got["private"][g]
                sc.clear()
        finally:
            sc.close()
            for s in sets:
                s.close()
    finally:
        tbl.close()


def test_a_stale_screen_refuses(ctx):
    """the plane belongs to one geometry of one table: a re-hash, an insert of new keys or a clear behind the handle"""
    from panagram_amd import engine
    keys = sample(K)[0]
    M = masks(8, NKEYS, seed=4)
    tbl = engine.PanTable(ctx, K, 8)
    ss = engine.SeqSet.from_host(ctx, sample(K)[1][0])
    try:
        load(tbl, keys[:-100], M[:-100])

        def refused(sc):
            for call in (lambda: sc.add(ss), lambda: sc.result(1)):
                with pytest.raises(engine.PanagramHipError) as ei:
                    call()
                assert ei.value.code == -1 and "changed behind the screen" in str(ei.value)
            sc.clear()  # (still the handle's own memory)
            sc.close()
        sc = engine.TableScreen(tbl)
        sc.add(ss)
        tbl.rehash(6.0)
        refused(sc)
        sc = engine.TableScreen(tbl)  # a new one answers
        sc.add(ss)
        same(sc.result(1), SR.screen(keys[:-100], M[:-100], SR.depths(keys[:-100], sample(K)[1][:1], K)[2], 1), "after the re-hash")
        load(tbl, keys[-100:], M[-100:])  # new keys
        refused(sc)
        sc = engine.TableScreen(tbl)
        tbl.clear()
        refused(sc)
        sc = engine.TableScreen(tbl)
        with pytest.raises(ValueError, match="min_count"):
            sc.result(0)
        with pytest.raises(ValueError, match="min_count"):
            sc.result(256)
        lib = ctx._lib
        assert lib.pg_screen_result(sc._h, 0, *[None] * 8, None) == -1 and b"min_count" in lib.pg_last_error()
        assert lib.pg_screen_result(sc._h, 256, *[None] * 8, None) == -1 and b"min_count" in lib.pg_last_error()
        assert lib.pg_screen_result(sc._h, 1, *[None] * 8, None) == 0  # (every output may be NULL)
        assert lib.pg_screen_add_seqset(sc._h, None, None, None) == -1 and b"NULL" in lib.pg_last_error()
        assert lib.pg_screen_create(None, None) == -1 and b"pg_screen_create" in lib.pg_last_error()
        sc.close()
        sc.close()
    finally:
        ss.close()
        tbl.close()


def test_the_table_closes_its_screens_first(ctx):
    from panagram_amd import engine
    tbl = engine.PanTable(ctx, K, 3)
    sc = engine.TableScreen(tbl)
    tbl.close()
    assert sc._h is None


def test_more_than_512_genomes_are_refused(ctx):
    from panagram_amd import engine
    wide = engine.PanTable(ctx, K, 513)
    try:
        sc = engine.TableScreen(wide)
        with pytest.raises(engine.PanagramHipError) as ei:
            sc.result(1)
        assert ei.value.code == -1 and "pg_screen_result" in str(ei.value) and "513 genomes" in str(ei.value)
        sc.close()
    finally:
        wide.close()


def test_an_empty_table_and_an_empty_sequence_set_give_zeros(ctx):
    from panagram_amd import engine
    keys, sets = sample(K)[0], sample(K)[1]
    for n in (5, 130):
        tbl = engine.PanTable(ctx, K, n)
        try:
            sc = engine.TableScreen(tbl)
            ss = engine.SeqSet.from_host(ctx, sets[0])
            windows, hits = sc.add(ss)
            ss.close()
            assert windows == SR.depths(keys, sets[:1], K)[0] and hits == 0
            got = sc.result(1)
            for f in FIELDS:
                assert got[f].shape == ((n,) if f in FIELDS[:4] else (n + 1,) if f in FIELDS[4:6] else (64,)) and not got[f].any(), (n, f)
            assert got["nkeys"] == 0
            sc.close()
        finally:
            tbl.close()
    M = masks(8, NKEYS, seed=5)
    tbl = engine.PanTable(ctx, K, 8)
    try:
        load(tbl, keys, M)
        sc = engine.TableScreen(tbl)
        empty, nreads, used = engine.SeqSet.from_fastq(ctx, b"")  # one contig of no base
        short = engine.SeqSet.from_host(ctx, [b"ACGT", b"N" * 30, b"ACGTACGTACGTACGTACGT"])  # no contig holds a window
        try:
            assert (nreads, used) == (0, 0) and sc.add(empty) == (0, 0) and sc.add(short) == (0, 0)
        finally:
            empty.close()
            short.close()
        same(sc.result(1), SR.screen(keys, M, np.zeros(len(keys), np.int64), 1), "nothing added")
        sc.close()
    finally:
        tbl.close()
