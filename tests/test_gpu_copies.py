"""GPU: the copy-number kernels (panagram_amd/csrc/pg_copies.hip) against the numpy model (tests/copies_ref.py), exactly:
k_copy_insert's distinct keys, k_copy_count's hits and counters — read back through the depth track — and k_copy_profile's
histograms, valid counts and tracks, at every edge the kernels have: a table whose probes wrap, a job edge, chunk edges, 64 lanes
on one counter."""
import ctypes as C

import numpy as np
import pytest

from tests import copies_ref as cr

pytestmark = pytest.mark.gpu

K = 21
JOB = 1 << 14
CHUNK = 4096
PG_E_INVALID, PG_E_CAPACITY = -1, -4
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def rand(rng, n):
    return bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)])


def revcomp(s):
    return s.translate(_COMP)[::-1]


def plane_sum(targets, track_row, k):
    """the sum of a plane's counters: the depth at the first position of every distinct key of the targets"""
    keys, at, off = [], [], 0
    for key, valid in cr.keys_of(targets, k):
        keys.append(key[valid])
        at.append(off + np.flatnonzero(valid))
        off += len(key)
    keys, at = np.concatenate(keys), np.concatenate(at)
    _, first = np.unique(keys, return_index=True)
    return int(track_row[at[first]].astype(np.int64).sum())


def held_to_model(ctx, targets, genomes, k=K, capacity=None):
    """one table for ``targets``, every genome into a plane of its own, one profile: all of it equal to the model's"""
    from panagram_amd import engine
    total = sum(max(0, len(t) - k + 1) for t in targets)
    tss = engine.SeqSet.from_host(ctx, targets)
    table = engine.CopyTable(ctx, k, capacity or max(1, total), len(genomes))
    try:
        assert table.insert(tss) == cr.distinct(targets, k)
        assert table.insert(tss) == 0  # (every key is there already)
        hits = []
        for g, contigs in enumerate(genomes):
            gss = engine.SeqSet.from_host(ctx, contigs)
            hits.append(table.count(g, gss))
            gss.close()
        assert hits == [cr.hits(targets, contigs, k) for contigs in genomes]
        hist, valid, track = table.profile(tss, track=True)
        whist, wvalid, wtrack = cr.profile(targets, genomes, k)
        assert np.array_equal(valid, wvalid)
        assert np.array_equal(track, wtrack), np.flatnonzero((track != wtrack).any(axis=0))[:10]
        assert np.array_equal(hist, whist)
        assert (hist.sum(axis=2) == valid[:, None]).all()
        if total and int(wtrack[wtrack != cr.DEPTH_INVALID].max(initial=0)) < cr.DEPTH_MAX:
            assert [plane_sum(targets, track[g], k) for g in range(len(genomes))] == hits
        h2, v2 = table.profile(tss)  # (without a track: the same histograms)
        assert np.array_equal(h2, hist) and np.array_equal(v2, valid)
    finally:
        table.close()
        tss.close()
    return hist, valid, track


def test_a_table_of_64_slots_where_probes_wrap(ctx):
    """32 distinct keys in 64 slots, eight sets of them: a key whose home is one of the last slots walks on at slot 0"""
    from panagram_amd import engine
    for seed in range(8):
        rng = np.random.default_rng(100 + seed)
        target = rand(rng, 32 + K - 1)
        assert cr.distinct([target], K) == 32
        genome = [rand(rng, 500) + target + rand(rng, 300) + revcomp(target)[5:] + rand(rng, 100)]
        hist, valid, _ = held_to_model(ctx, [target], [genome], capacity=32)
        assert valid.tolist() == [32] and hist[0, 0, 2] >= 27
    # capacity 1: two slots, one key — the homopolymer's
    held_to_model(ctx, [b"A" * 30], [[b"T" * 50 + b"C" + b"A" * 25]], capacity=1)
    del engine


def test_capacity_exceeded_is_an_error_that_stays(ctx):
    from panagram_amd import engine
    rng = np.random.default_rng(7)
    big, small = engine.SeqSet.from_host(ctx, [rand(rng, 400)]), engine.SeqSet.from_host(ctx, [rand(rng, K + 2)])
    table = engine.CopyTable(ctx, K, 8, 1)  # 16 slots
    try:
        assert table.insert(small) == 3
        with pytest.raises(engine.PanagramHipError) as e:
            table.insert(big)
        assert e.value.code == PG_E_CAPACITY
        for call in (lambda: table.insert(small), lambda: table.count(0, small), lambda: table.profile(small)):
            with pytest.raises(engine.PanagramHipError) as e:
                call()
            assert e.value.code == PG_E_CAPACITY
    finally:
        table.close()
        big.close()
        small.close()


def test_distinct_keys_accumulate_over_inserts(ctx):
    from panagram_amd import engine
    rng = np.random.default_rng(8)
    a, b = rand(rng, 3000), rand(rng, 2000)
    first = [a, a[100:900], revcomp(a[:500]), b"ACGTN" * 10, b"ACG"]
    second = [b, a[2000:], b[:700].lower()]
    table = engine.CopyTable(ctx, K, 6000, 1)
    s1, s2 = engine.SeqSet.from_host(ctx, first), engine.SeqSet.from_host(ctx, second)
    try:
        n1 = table.insert(s1)
        assert n1 == cr.distinct(first, K) == len(np.unique(cr.valid_keys(first, K)))
        assert table.insert(s2) == cr.distinct(first + second, K) - n1
        assert table.insert(s1) == 0
    finally:
        table.close()
        s1.close()
        s2.close()


def test_three_contigs_a_job_edge_a_short_one_and_n(ctx):
    rng = np.random.default_rng(9)
    gene = rand(rng, 1500)
    # contig 0: one job of k-mer positions and five more, a copy of the gene astride the job's edge
    c0 = rand(rng, JOB - 1490) + gene + rand(rng, 5 + K - 1 - 10)
    assert len(c0) - K + 1 == JOB + 5
    c1 = gene[:K - 1]
    c2 = rand(rng, 300) + gene[:600] + b"N" + gene[601:] + rand(rng, 200) + b"NNNN" + revcomp(gene)
    hist, valid, track = held_to_model(ctx, [gene, gene[700 - 30:700 + 30]], [[c0, c1, c2]])
    assert hist[0, 0, 3] == 1500 - K + 1 - K and hist[0, 0, 2] == K  # (three copies, one of them cut by an N)


def test_homopolymer_and_satellite_are_counted_exactly(ctx):
    """all 64 lanes of a wave on one counter (A x 5000), and on three (ACG x 1700); a depth above the track's cap"""
    rng = np.random.default_rng(10)
    genome = [rand(rng, 3000) + b"A" * 5000 + rand(rng, 1000) + b"ACG" * 1700 + rand(rng, 2000), b"T" * 300 + rand(rng, 100) + b"GTC" * 50]
    targets = [b"A" * 100, b"ACG" * 40, b"CGT" * 40, rand(rng, 200), b"T" * 40]
    hist, valid, track = held_to_model(ctx, targets, [genome])
    assert hist[0, 0, 63] == 100 - K + 1 and int(track[0, 0]) >= 5000 - K + 1 + 300 - K + 1
    assert hist[1, 0, 63] == 120 - K + 1 and int(track[0, 80:80 + 100].min()) >= 1690
    long_run = [b"C" + b"A" * 70000 + b"G"]
    hist, valid, track = held_to_model(ctx, [b"A" * 30], [long_run])
    assert (track == cr.DEPTH_MAX).all() and hist[0, 0, 63] == 10


def test_planes_are_independent(ctx):
    from panagram_amd import engine
    rng = np.random.default_rng(11)
    gene = rand(rng, 2000)
    ga, gb = [rand(rng, 800) + gene + rand(rng, 500) + gene[300:1200]], [gene[1000:] + rand(rng, 700)]
    tss, sa, sb = (engine.SeqSet.from_host(ctx, x) for x in ([gene], ga, gb))
    table = engine.CopyTable(ctx, K, 2000, 3)
    try:
        table.insert(tss)
        ha, hb = table.count(0, sa), table.count(2, sa)
        assert ha == hb == cr.hits([gene], ga, K)
        _, _, t = table.profile(tss, track=True)
        want = cr.profile([gene], [ga, gb], K)[2]
        assert np.array_equal(t[0], want[0]) and np.array_equal(t[2], want[0]) and not t[1].any()
        table.count(0, sa)  # twice into one plane: doubled
        table.count(1, sb)
        hist, valid, t = table.profile(tss, track=True)
        assert np.array_equal(t[0], 2 * want[0]) and np.array_equal(t[1], want[1]) and np.array_equal(t[2], want[0])
        # a plane range that starts above 0
        h12, v12, t12 = table.profile(tss, 1, 2, track=True)
        assert np.array_equal(h12, hist[:, 1:]) and np.array_equal(v12, valid) and np.array_equal(t12, t[1:])
        h2, _ = table.profile(tss, 2)
        assert np.array_equal(h2, hist[:, 2:])
        table.clear(0)
        hist, _, t = table.profile(tss, track=True)
        assert not t[0].any() and hist[0, 0, 0] == valid[0] and np.array_equal(t[1], want[1]) and np.array_equal(t[2], want[0])
    finally:
        table.close()
        for s in (tss, sa, sb):
            s.close()


def test_chunk_edges_of_the_profile(ctx):
    rng = np.random.default_rng(12)
    src = rand(rng, 30000)
    sizes = [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK]
    targets, at = [], 0
    for n in sizes:  # (the targets overlap: a window that two of them share reads one depth)
        targets.append(src[at:at + n + K - 1])
        at += n // 2 + 100
    targets.append(src[5000:5000 + CHUNK + K - 1 - 300] + b"N" + src[5000 + CHUNK + K - 300:5000 + CHUNK + K + 50])  # an N astride the edge
    genome = [src[:20000] + rand(rng, 5000) + revcomp(src[2000:9000])]
    hist, valid, track = held_to_model(ctx, targets, [genome, [rand(rng, 1000)]])
    assert valid[:5].tolist() == sizes and hist[:, 1, 0].tolist() == valid.tolist()


def test_a_set_that_was_never_inserted_reads_depth_0(ctx):
    from panagram_amd import engine
    rng = np.random.default_rng(13)
    gene, other = rand(rng, 900), [rand(rng, 5000) + b"NN" + rand(rng, 50), rand(rng, 10), b""]
    tss, oss = engine.SeqSet.from_host(ctx, [gene]), engine.SeqSet.from_host(ctx, other)
    gss = engine.SeqSet.from_host(ctx, [gene + other[0]])
    table = engine.CopyTable(ctx, K, 900, 1)
    try:
        table.insert(tss)
        table.count(0, gss)
        hist, valid, track = table.profile(oss, track=True)
        n0 = len(other[0]) - K + 1
        assert valid.tolist() == [n0 - (K + 1), 0, 0] and hist[0, 0, 0] == valid[0] and hist[:, :, 1:].sum() == 0
        want = cr.profile(other, [[b""]], K)[2]
        assert np.array_equal(track, want) and (track == cr.DEPTH_INVALID).sum() == K + 1
    finally:
        table.close()
        for s in (tss, oss, gss):
            s.close()


def test_invalid_arguments(ctx):
    from panagram_amd import engine
    lib = ctx._lib
    rng = np.random.default_rng(14)
    ss = engine.SeqSet.from_host(ctx, [rand(rng, 100)])
    other_ctx = engine.Context(0)
    foreign = engine.SeqSet.from_host(other_ctx, [rand(rng, 100)])
    table = engine.CopyTable(ctx, K, 100, 2)
    h, n = C.c_void_p(), C.c_uint64()
    hist, valid = np.zeros((1, 2, 64), np.uint64), np.zeros(1, np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    try:
        calls = [
            lambda: lib.pg_copytable_create(ctx._h, 0, 100, 1, C.byref(h)),
            lambda: lib.pg_copytable_create(ctx._h, 33, 100, 1, C.byref(h)),
            lambda: lib.pg_copytable_create(ctx._h, K, 0, 1, C.byref(h)),
            lambda: lib.pg_copytable_create(ctx._h, K, 100, 0, C.byref(h)),
            lambda: lib.pg_copytable_create(None, K, 100, 1, C.byref(h)),
            lambda: lib.pg_copytable_create(ctx._h, K, 100, 1, None),
            lambda: lib.pg_copytable_insert_seqset(None, ss._h, C.byref(n)),
            lambda: lib.pg_copytable_insert_seqset(table._h, None, C.byref(n)),
            lambda: lib.pg_copytable_insert_seqset(table._h, ss._h, None),
            lambda: lib.pg_copytable_insert_seqset(table._h, foreign._h, C.byref(n)),
            lambda: lib.pg_copytable_count_seqset(table._h, 2, ss._h, C.byref(n)),
            lambda: lib.pg_copytable_count_seqset(table._h, 0, None, C.byref(n)),
            lambda: lib.pg_copytable_count_seqset(table._h, 0, ss._h, None),
            lambda: lib.pg_copytable_count_seqset(table._h, 0, foreign._h, C.byref(n)),
            lambda: lib.pg_copytable_clear_plane(table._h, 2),
            lambda: lib.pg_copytable_clear_plane(None, 0),
            lambda: lib.pg_copytable_profile(table._h, ss._h, 0, 3, p(hist), p(valid), None),
            lambda: lib.pg_copytable_profile(table._h, ss._h, 2, 1, p(hist), p(valid), None),
            lambda: lib.pg_copytable_profile(table._h, ss._h, 1, 2, p(hist), p(valid), None),
            lambda: lib.pg_copytable_profile(table._h, ss._h, 0, 0, p(hist), p(valid), None),
            lambda: lib.pg_copytable_profile(table._h, ss._h, 0, 2, None, p(valid), None),
            lambda: lib.pg_copytable_profile(table._h, ss._h, 0, 2, p(hist), None, None),
            lambda: lib.pg_copytable_profile(table._h, None, 0, 2, p(hist), p(valid), None),
            lambda: lib.pg_copytable_profile(table._h, foreign._h, 0, 2, p(hist), p(valid), None),
            lambda: lib.pg_copies_last_timing(None),
        ]
        for i, call in enumerate(calls):
            assert call() == PG_E_INVALID, i
            assert lib.pg_last_error()
        assert lib.pg_copytable_destroy(None) == 0
        # and the table is none the worse for it
        assert table.insert(ss) == 80 and table.count(1, ss) == 80
        assert set(engine.copies_last_timing()) == {"insert_ms", "count_ms", "profile_ms"}
    finally:
        table.close()
        foreign.close()
        other_ctx.close()
        ss.close()


def test_two_megabases_three_genomes(ctx):
    """more than one wave of blocks: 3 x 2 Mb of genome (123 jobs each) against 50 kb of targets"""
    rng = np.random.default_rng(15)
    targets = [rand(rng, n) for n in (20000, 12000, 9000, 5000, 3000, 1000)]
    assert sum(len(t) for t in targets) == 50000

    def genome(copies, seed):
        r = np.random.default_rng(seed)
        parts = [rand(r, 1_900_000 // (len(copies) + 1)) for _ in range(len(copies) + 1)]
        out = [parts[0]]
        for c, f in zip(copies, parts[1:]):
            out += [c, f]
        seq = b"".join(out)
        return [seq[:1_200_000], seq[1_200_000:]]
    t = targets
    genomes = [genome([t[0], t[1], revcomp(t[1]), t[2]] + [t[4]] * 6, 1), genome([t[0][:8000], t[3], t[3], t[3], revcomp(t[5])], 2),
               genome([t[2][100:4000]] * 70, 3)]
    hist, valid, track = held_to_model(ctx, targets, genomes)
    from panagram_amd import copies as cp
    med = cp.lower_median(hist)
    assert med[:, 0].tolist() == [1, 2, 1, 0, 6, 0] and med[:, 1].tolist() == [0, 0, 0, 3, 0, 1] and med[:, 2].tolist() == [0, 0, 0, 0, 0, 0]
    assert hist[2, 2, 63] == 3900 - K + 1
