"""GPU: engine.PanTable.kmer_stats (k_table_pair_counts) — the pan table's shared distinct k-mer counts against the numpy
reference (tests/kmerstats_ref.py), exactly: crafted masks at every layout and mask width, sparse and dense tables, a re-hash,
tables built from sequence (retired slots among them), an empty table, and the entry point's errors."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import kmerstats_ref as KR

pytestmark = pytest.mark.gpu

K = 21
NKEYS = 3000
# every layout and every W up to 7: slots (W = 1: 1, 7, 8, 32; W = 2: 33, 64), inline (W = 3: 65, 96), split (W = 4..7)
WIDTHS = [1, 7, 8, 32, 33, 64, 65, 96, 97, 128, 129, 200]


def crafted(n, nkeys=NKEYS, seed=0):
    """(keys, M): all-ones keys, one key private to every genome (bit n - 1 among them), keys whose only bits lie in the last
    32-genome word, random masks of every density for the rest; no key without a bit"""
    rng = np.random.default_rng(1000 * n + seed)
    keys = KR.random_keys(rng, nkeys, K)
    M = (rng.random((nkeys, n)) < rng.random((nkeys, 1))).astype(np.uint8)
    M[:10] = 1
    M[10:10 + n] = np.eye(n, dtype=np.uint8)
    last0 = 32 * ((n - 1) // 32)
    tail = M[10 + n: 30 + n]
    tail[:, :last0] = 0
    tail[:, n - 1] |= (tail[:, last0:].sum(axis=1) == 0).astype(np.uint8)
    none = M.sum(axis=1) == 0
    M[none, rng.integers(0, n, int(none.sum()))] = 1
    return keys, M


def load(tbl, keys, M):
    """through PanTable.insert_keys: one call per 32-genome group, with the keys whose word is non-zero there"""
    for d, words in enumerate(KR.group_words(M)):
        has = words != 0
        tbl.insert_keys(d, keys[has], words[has])


def same(got, ref, tag):
    assert got["pairs"].dtype == np.int64 and got["pairs"].shape == ref["pairs"].shape, tag
    bad = np.argwhere(got["pairs"] != ref["pairs"])
    assert len(bad) == 0, (tag, "pairs", len(bad), bad[:5].tolist(), [int(got["pairs"][tuple(b)]) for b in bad[:5]],
                           [int(ref["pairs"][tuple(b)]) for b in bad[:5]])
    assert np.array_equal(got["pairs"], got["pairs"].T), tag
    assert got["occupancy"].tolist() == ref["occupancy"].tolist(), (tag, "occupancy")
    assert got["private"].tolist() == ref["private"].tolist(), (tag, "private")
    assert got["nkeys"] == ref["nkeys"], (tag, "nkeys", got["nkeys"], ref["nkeys"])


@pytest.fixture(scope="module")
def references():
    """(keys, M, reference) per genome count, computed once and left alone"""
    out = {}
    for n in WIDTHS:
        keys, M = crafted(n)
        out[n] = (keys, M, KR.stats(keys, M))
    return out


@pytest.mark.parametrize("n", WIDTHS)
def test_crafted_masks_at_every_layout_and_width(ctx, references, n):
    from panagram_amd import engine
    keys, M, ref = references[n]
    assert ref["occupancy"][n] >= 10 and (ref["private"] >= 1).all() and ref["occupancy"][0] == 0
    tbl = engine.PanTable(ctx, K, n)
    try:
        load(tbl, keys, M)
        got = tbl.kmer_stats()
        same(got, ref, n)
        assert got["nkeys"] == tbl.stats()["nkeys"] == NKEYS
        again = tbl.kmer_stats()  # a second call: the same arrays
        for name in ("pairs", "occupancy", "private"):
            assert np.array_equal(again[name], got[name]), (n, name)
        assert again["nkeys"] == got["nkeys"]
    finally:
        tbl.close()


@pytest.mark.parametrize("n", [40, 41, 512])
def test_widths_at_which_the_kernel_changes_its_path(ctx, n):
    """40 / 41 genomes: the last width whose 4 x 4 blocks are one per lane of a wave, and the first that takes three rounds;
    512: the widest, eleven slices of blocks and the most LDS"""
    from panagram_amd import engine
    keys, M = crafted(n)
    ref = KR.stats(keys, M)
    tbl = engine.PanTable(ctx, K, n)
    try:
        load(tbl, keys, M)
        same(tbl.kmer_stats(), ref, n)
        tbl.rehash(6.0)
        same(tbl.kmer_stats(), ref, (n, "dense"))
    finally:
        tbl.close()


@pytest.mark.parametrize("n", [8, 97])
def test_sparse_and_dense_tables(ctx, references, n):
    """a table created for 100 x the keys (most tiles hold no key), and one re-hashed so dense that groups spill past their
    home line"""
    from panagram_amd import engine
    keys, M, ref = references[n]
    tbl = engine.PanTable(ctx, K, n, expected_keys=100 * NKEYS)
    try:
        load(tbl, keys, M)
        st = tbl.stats()
        assert st["nslots"] > 100 * NKEYS
        same(tbl.kmer_stats(), ref, (n, "sparse", st["nslots"]))
        tbl.rehash(6.0)
        spilled, slots = tbl.spill()
        assert spilled > 0.02 and tbl.stats()["nslots"] < 2 * NKEYS, (spilled, tbl.stats())
        same(tbl.kmer_stats(), ref, (n, "dense", spilled, slots))
    finally:
        tbl.close()


def test_dense_table_of_more_tiles_than_blocks(ctx):
    """600 000 keys at 6 per line: more than 2048 tiles, every one full — a block takes several, through both tile buffers"""
    from panagram_amd import engine
    n = 8
    keys, M = crafted(n, 600_000, seed=1)
    ref = KR.stats(keys, M)
    tbl = engine.PanTable(ctx, K, n, expected_keys=len(keys))
    try:
        load(tbl, keys, M)
        tbl.rehash(6.0)
        assert tbl.stats()["nslots"] > 2048 * 256
        same(tbl.kmer_stats(), ref, "600k keys")
    finally:
        tbl.close()


@pytest.mark.parametrize("n", [33, 65, 129])
def test_a_rehash_changes_nothing(ctx, references, n):
    from panagram_amd import engine
    keys, M, ref = references[n]
    tbl = engine.PanTable(ctx, K, n)
    try:
        load(tbl, keys, M)
        before = tbl.kmer_stats()
        tbl.rehash(2.0)
        after = tbl.kmer_stats()
        same(before, ref, (n, "before"))
        same(after, ref, (n, "after"))
    finally:
        tbl.close()


def _from_sequence(ctx, genomes):
    from panagram_amd import engine
    n = len(genomes)
    keys, M = KR.from_groups(po.build_bitvec_dbs(genomes, K), n)
    ref = KR.stats(keys, M)
    tbl = engine.PanTable(ctx, K, n)
    try:
        for g in range(n):
            ss = engine.SeqSet.from_host(ctx, genomes[g])
            tbl.insert_seqset(g, ss)
            ss.close()
        got = tbl.kmer_stats()
        same(got, ref, "from sequence")
        assert got["nkeys"] == tbl.stats()["nkeys"]
    finally:
        tbl.close()
    return ref


def test_table_built_from_sequence(ctx):
    genomes = [[po.codes_to_ascii(c) for c in g] for g in po.synth_genomes(8, [20000], 0.02, 5)]
    ref = _from_sequence(ctx, genomes)
    assert ref["occupancy"][8] > 1000 and ref["private"][1:].min() > 100  # the input stays non-trivial (genome 0 is the ancestor)


def test_repeat_family_retired_slots_are_not_counted(ctx):
    """many diverged copies of one element (tools/repeat_stress.py's generator): the build's racing claims leave retired
    slots behind, and no key may be counted twice"""
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
    _from_sequence(ctx, genomes)


def test_empty_table_gives_zeros(ctx):
    from panagram_amd import engine
    for n in (5, 130):
        tbl = engine.PanTable(ctx, K, n)
        try:
            got = tbl.kmer_stats()
            assert got["pairs"].shape == (n, n) and not got["pairs"].any()
            assert got["occupancy"].shape == (n + 1,) and not got["occupancy"].any()
            assert got["private"].shape == (n,) and not got["private"].any() and got["nkeys"] == 0
        finally:
            tbl.close()


def test_error_codes_and_messages(ctx):
    from panagram_amd import engine
    lib = ctx._lib
    tbl = engine.PanTable(ctx, K, 4)
    try:
        out = np.zeros(16, np.uint64)
        assert lib.pg_table_pair_counts(tbl._h, None, None, None, None) == -1  # PG_E_INVALID
        assert b"pg_table_pair_counts" in lib.pg_last_error() and b"NULL" in lib.pg_last_error()
        assert lib.pg_table_pair_counts(None, out.ctypes.data_as(C.c_void_p), None, None, None) == -1
        assert b"pg_table_pair_counts" in lib.pg_last_error()
        # occ, priv and nkeys may be NULL
        assert lib.pg_table_pair_counts(tbl._h, out.ctypes.data_as(C.c_void_p), None, None, None) == 0
    finally:
        tbl.close()
    wide = engine.PanTable(ctx, K, 513)
    try:
        with pytest.raises(engine.PanagramHipError) as ei:
            wide.kmer_stats()
        assert ei.value.code == -1 and "pg_table_pair_counts" in str(ei.value) and "513 genomes" in str(ei.value)
    finally:
        wide.close()
