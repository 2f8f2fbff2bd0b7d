"""GPU: the synteny kernels (panagram_amd/csrc/pg_synteny.hip) against the numpy model (tests/synteny_ref.py), exactly — order
included.  k_mate_runs on crafted arrays of mate words (no hashing involved): a wave takes 64 positions, a tile 256, a
workgroup's chunk 4096.  k_pos_insert / k_pos_mates on sequences with repeats, palindromes, N runs and short contigs.
pg_synteny_segments, all of it in one call, on diverged and on rearranged genomes."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import synteny_ref as sr

pytestmark = pytest.mark.gpu

NO = sr.NO_MATE
CHUNK = 4096
PG_E_INVALID, PG_E_CAPACITY = -1, -4


def _put(m, a, b, pos, strand):
    """positions [a, b) of one contig's array mated from posB = pos on, ascending on strand 0, descending on strand 1"""
    j = np.arange(b - a, dtype=np.int64)
    m[a:b] = ((pos + j) << 1) if strand == 0 else (((pos - j) << 1) | 1)


def _crafted():
    """(mates, nkmers): one array of many contigs, every edge the kernel has in one of them"""
    contigs = []
    c = np.full(3 * CHUNK + 77, NO, np.int64)        # a run ending at 4095, one starting at 4096, one spanning 8191 - 8192 on
    _put(c, 10, CHUNK, 5, 0)                         # strand -, one to the contig's last position
    _put(c, CHUNK, CHUNK + 4, 70000, 0)
    _put(c, 8000, 8200, 900000, 1)
    _put(c, 3 * CHUNK, 3 * CHUNK + 77, 123, 0)
    contigs.append(c)
    c = np.full(2 * CHUNK, NO, np.int64)             # one run filling two chunks whole
    _put(c, 0, 2 * CHUNK, 50000, 1)
    contigs.append(c)
    c = np.full(CHUNK, NO, np.int64)                 # one chunk, whole
    _put(c, 0, CHUNK, 1 << 20, 0)
    contigs.append(c)
    c = np.full(1000, NO, np.int64)                  # ends at 63 / starts at 64, ends at 255 / starts at 256, a single position
    _put(c, 0, 64, 0, 0)
    _put(c, 64, 70, 64 + 1, 0)                       # (posB jumps by 2 at position 64: a new run)
    _put(c, 100, 256, 5000, 1)
    _put(c, 256, 300, 7000, 1)
    _put(c, 320, 321, 9, 0)
    contigs.append(c)
    c = np.full(700, NO, np.int64)                   # spanning 63 - 64 and 255 - 256; the three breaks inside mated stretches
    _put(c, 60, 70, 11, 0)
    _put(c, 250, 260, 400, 1)
    _put(c, 300, 310, 1000, 0)
    _put(c, 310, 320, 1011, 0)                       # posB + 2
    _put(c, 400, 410, 2000, 0)
    _put(c, 410, 420, 2008, 0)                       # posB - 1 on strand +
    _put(c, 500, 510, 3000, 0)
    _put(c, 510, 520, 3010, 1)                       # a strand flip at the consecutive posB
    _put(c, 600, 610, 4000, 1)
    _put(c, 610, 620, 3991, 0)                       # ... and the other way round
    _put(c, 640, 650, 4100, 1)
    _put(c, 650, 660, 4091, 1)                       # posB + 1 on strand -
    contigs.append(c)
    contigs.append(np.zeros(0, np.int64))            # contigs of 0, 1 (mated), 1 (not) and 4097 positions
    contigs.append(np.array([42 << 1], np.int64))
    contigs.append(np.array([NO], np.int64))
    c = np.full(CHUNK + 1, NO, np.int64)
    _put(c, CHUNK - 1, CHUNK + 1, 77, 1)             # the last two positions: across the chunk edge, to the contig's end
    contigs.append(c)
    c = np.full(CHUNK + 1, NO, np.int64)
    _put(c, 0, CHUNK + 1, 10 ** 6, 0)
    contigs.append(c)
    c = np.full(100, NO, np.int64)                   # two contigs of A adjacent in B: the words go on without a break
    _put(c, 0, 100, 300, 0)
    contigs.append(c)
    c = np.full(50, NO, np.int64)
    _put(c, 0, 50, 400, 0)
    contigs.append(c)
    contigs.append(np.zeros(0, np.int64))
    contigs.append(np.full(5000, NO, np.int64))      # no mate at all
    c = np.full(3, NO, np.int64)                     # the largest words: 0xFFFFFFFE is a mate, nothing wraps
    c[:] = [NO - 3, NO - 1, NO]
    contigs.append(c)
    return np.concatenate(contigs).astype(np.uint32), [len(c) for c in contigs]


def _same_runs(got, want, tag=""):
    rc, rs, re_, rm, per = got[:5]
    assert len(rc) == len(want), (tag, len(rc), len(want))
    assert np.array_equal(np.stack([rc, rs, re_, rm], axis=1).astype(np.int64), want), tag
    ncontigs = len(per)
    assert np.array_equal(per.astype(np.int64), np.bincount(want[:, 0], minlength=ncontigs)[:ncontigs]), tag


def test_mate_runs_on_crafted_arrays(ctx):
    from panagram_amd import engine
    m, nk = _crafted()
    want = sr.runs(m, nk)
    # what the crafted array is there for, stated once by hand: the edges of contig 0 and the adjacent contigs
    assert want[:4].tolist() == [[0, 10, CHUNK, 10], [0, CHUNK, CHUNK + 4, 140000], [0, 8000, 8200, 1800001], [0, 3 * CHUNK, 3 * CHUNK + 77, 246]]
    assert [r for r in want.tolist() if r[0] in (10, 11)] == [[10, 0, 100, 600], [11, 0, 50, 800]]
    assert len(want[want[:, 0] == 4]) == 12 and want[-1].tolist() == [14, 0, 2, NO - 3]
    _same_runs(engine.mate_runs(ctx, m, nk), want)
    # the same on every call
    a, b = engine.mate_runs(ctx, m, nk), engine.mate_runs(ctx, m, nk)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_mate_runs_capacity_protocol(ctx):
    from panagram_amd import engine
    m, nk = _crafted()
    want = sr.runs(m, nk)
    total = len(want)
    per_want = np.bincount(want[:, 0], minlength=len(nk))
    for cap in (0, total - 1):
        *arrs, per, got_total = engine.mate_runs(ctx, m, nk, cap=cap)
        assert got_total == total and np.array_equal(per.astype(np.int64), per_want), cap
        assert all((a == NO).all() for a in arrs), cap  # nothing is written
    *arrs, per, got_total = engine.mate_runs(ctx, m, nk, cap=total)
    assert got_total == total
    _same_runs((*arrs, per), want, "cap = total")
    *arrs, per, got_total = engine.mate_runs(ctx, m, nk, cap=total + 5)
    _same_runs((*[a[:total] for a in arrs], per), want, "cap > total")
    assert all((a[total:] == NO).all() for a in arrs)


def test_mate_runs_all_unmated_empty_and_random(ctx):
    from panagram_amd import engine
    got = engine.mate_runs(ctx, np.full(9000, NO, np.uint32), [9000])
    assert all(len(a) == 0 for a in got[:4]) and got[4].tolist() == [0]
    got = engine.mate_runs(ctx, np.zeros(0, np.uint32), [])
    assert all(len(a) == 0 for a in got)
    got = engine.mate_runs(ctx, np.zeros(0, np.uint32), [0, 0])
    assert got[4].tolist() == [0, 0]
    # random stretches of every kind, three contigs
    rng = np.random.default_rng(17)
    nk = [20011, 1, 13000]
    m = np.full(sum(nk), NO, np.int64)
    at = 0
    while at < len(m):
        n = int(rng.choice([1, 2, 3, 63, 64, 65, 200, 300, 1000])) if rng.random() < 0.7 else int(rng.integers(1, 40))
        n = min(n, len(m) - at)
        if rng.random() < 0.6:
            strand = int(rng.integers(0, 2))
            _put(m, at, at + n, int(rng.integers(10000, 1 << 30)), strand)
        at += n
    m = m.astype(np.uint32)
    want = sr.runs(m, nk)
    assert len(want) > 100
    _same_runs(engine.mate_runs(ctx, m, nk), want)


def test_mate_runs_invalid_sizes(ctx):
    from panagram_amd import engine
    lib = ctx._lib
    m = np.zeros(4, np.uint32)
    total = C.c_uint64()
    for nks in ([1 << 31], [1 << 30, 1 << 30], [(1 << 31) - 1, 1]):
        nk = np.array(nks, np.uint64)
        per = np.zeros(len(nk), np.uint64)
        rc = lib.pg_mate_runs(ctx._h, engine._ptr(m), len(nk), engine._ptr(nk), 0, None, None, None, None, engine._ptr(per), C.byref(total))
        assert rc == PG_E_INVALID, nks
    nk, per = np.array([4], np.uint64), np.zeros(1, np.uint64)
    assert lib.pg_mate_runs(ctx._h, engine._ptr(m), 1, engine._ptr(nk), 0, None, None, None, None, engine._ptr(per), None) == PG_E_INVALID
    assert lib.pg_mate_runs(ctx._h, engine._ptr(m), 1, engine._ptr(nk), 3, None, None, None, None, engine._ptr(per), C.byref(total)) == PG_E_INVALID
    with pytest.raises(ValueError):
        engine.mate_runs(ctx, m, [5])


# ---------------------------------------------------------------------------
# the table and the mates
# ---------------------------------------------------------------------------
def _gpu_mates(ctx, a, b, k, capacity=None):
    from panagram_amd import engine
    ssa, ssb = engine.SeqSet.from_host(ctx, a), engine.SeqSet.from_host(ctx, b)
    try:
        cap = capacity if capacity is not None else max(1, ssa.total_kmers(k) + ssb.total_kmers(k))
        pt = engine.PosTable(ctx, k, cap)
        try:
            pt.insert(0, ssa)
            pt.insert(1, ssb)
            return pt.mates(ssa)
        finally:
            pt.close()
    finally:
        ssa.close()
        ssb.close()


def _check_mates(ctx, a, b, k, capacity=None, tag=""):
    got, nmated = _gpu_mates(ctx, a, b, k, capacity)
    want, nk = sr.mates(a, b, k)
    assert got.dtype == np.uint32 and len(got) == sum(nk), tag
    assert np.array_equal(got, want), (tag, k, np.flatnonzero(got != want)[:10])
    assert nmated == int((want != NO).sum()), tag
    return want


@pytest.mark.parametrize("k", [5, 21, 31, 32])
def test_mates_equal_the_model(ctx, k):
    """two contigs per side over more than one job, B diverged from A; at k = 5 nearly every key occurs more than once"""
    a0, b0 = po.synth_genomes(2, [20000, 3011], 0.02, 40 + k)
    a = [sr.ascii_of(c) for c in a0]
    b = [sr.ascii_of(c) for c in b0][::-1]  # (B's contigs in the other order: posB is a global offset)
    want = _check_mates(ctx, a, b, k)
    if k >= 21:
        assert (want != NO).sum() > 5000
    else:
        assert (want != NO).sum() < 100


def test_even_k_palindromes_have_rc_zero(ctx):
    want = _check_mates(ctx, [b"GGACGTCC"], [b"TTACGTAA"], 4)
    assert want.tolist() == [NO, NO, 2 << 1, NO, NO]
    _check_mates(ctx, [b"AACCGTTTTGGAC"], [b"AACC"], 4)
    want = _check_mates(ctx, [b"AACCGGGTTGGAC"], [b"AACC"], 4)
    assert want[0] == NO
    s = sr.ascii_of(sr.random_codes(400, 21))
    _check_mates(ctx, [s], [s[::-1], s[50:90]], 4)
    _check_mates(ctx, [s], [s], 6)


def test_two_and_three_occurrences_and_one_on_each_strand(ctx):
    k = 21
    s = sr.random_codes(2000, 22)
    a = [s, s[100:200], s[300:400], s[300:400], sr.revcomp(s[600:700])]
    a = [sr.ascii_of(c) for c in a]
    b = [sr.ascii_of(s)]
    want = _check_mates(ctx, a, b, k)
    none = np.zeros(2000 - k + 1, bool)
    for lo in (100, 300, 600):
        none[lo:lo + 100 - k + 1] = True
    assert np.array_equal(want[:2000 - k + 1] == NO, none) and (want[2000 - k + 1:] == NO).all()
    # the same repeats on B's side: MULTI in B's field
    want = _check_mates(ctx, b, a, k)
    assert np.array_equal(want == NO, none)
    # and on both sides at once
    _check_mates(ctx, a, a, k)


def test_n_runs_lower_case_and_short_contigs(ctx):
    k = 21
    s = bytearray(sr.ascii_of(sr.random_codes(3000, 23)))
    s[500:530] = b"N" * 30
    s[1000] = ord("n")
    s[1500:1502] = b"RY"
    low = bytes(s).lower()
    a = [bytes(s), bytes(s[:k - 1]), bytes(s[40:40 + k]), b"A", low[2000:2600]]
    b = [low, bytes(s[:k]), b"ACGTN"]
    want = _check_mates(ctx, a, b, k)
    assert (want[500 - k + 1:530] == NO).all() and (want[1000 - k + 1:1001] == NO).all() and want[499 - k] != NO
    _check_mates(ctx, b, a, k)
    # a side without a single k-mer
    got, nmated = _gpu_mates(ctx, [b"ACGT"], [bytes(s)], k)
    assert len(got) == 0 and nmated == 0
    got, nmated = _gpu_mates(ctx, [bytes(s)], [b"ACGT", b"NNNNNNNNNNNNNNNNNNNNNNNNNNNNNN"], k)
    assert (got == NO).all() and nmated == 0


def test_table_at_its_minimum_size_with_clustered_keys(ctx):
    """no key shared between the sides: as many distinct keys as the table was created for.  Low-complexity sequence: the keys
    of a two-letter alphabet are close together as numbers"""
    k = 21
    rng = np.random.default_rng(24)
    a = [sr.ascii_of(rng.integers(0, 2, 6000).astype(np.uint8))]          # A / C only
    b = [sr.ascii_of((rng.integers(0, 2, 5000) * 2).astype(np.uint8))]    # A / G only
    for cap in (6000 - k + 1 + 5000 - k + 1, 8192, 8193):
        _check_mates(ctx, a, b, k, capacity=cap, tag=cap)
    _check_mates(ctx, a, a, k, capacity=2 * (6000 - k + 1))
    # 32 distinct keys in 64 slots, eight sets of them: a key whose home is one of the last slots walks on at slot 0, in the
    # insert of either side and in the lookup.  Against itself (every position mated, strand +) and its reverse complement (strand -)
    for seed in range(8):
        codes = sr.random_codes(32 + k - 1, 100 + seed)
        s, rc = sr.ascii_of(codes), sr.ascii_of(sr.revcomp(codes))
        assert len(np.unique(sr.side_kmers([s], k)[0])) == 32, seed
        for other in (s, rc):
            want = _check_mates(ctx, [s], [other], k, capacity=32, tag=("64 slots", seed, other is rc))
            assert (want != NO).all() and (want & 1 == (other is rc)).all(), seed
    # capacity 1: two slots, one key — the homopolymer's, held ten times by each side: no mate
    want = _check_mates(ctx, [b"A" * 30], [b"A" * 30], k, capacity=1, tag="two slots")
    assert len(want) == 10 and (want == NO).all()


def test_capacity_too_small_is_an_error_code(ctx):
    from panagram_amd import engine
    k = 21
    s = sr.ascii_of(sr.random_codes(3000, 25))
    ss = engine.SeqSet.from_host(ctx, [s])
    try:
        pt = engine.PosTable(ctx, k, 8)  # 16 slots for 2980 distinct keys
        with pytest.raises(engine.PanagramHipError) as ei:
            pt.insert(0, ss)
        assert ei.value.code == PG_E_CAPACITY
        for call in (lambda: pt.insert(1, ss), lambda: pt.mates(ss)):  # the table answers nothing any more
            with pytest.raises(engine.PanagramHipError) as ei:
                call()
            assert ei.value.code == PG_E_CAPACITY
        pt.close()
        # the context is as good as before
        want, _ = sr.mates([s], [s], k)
        pt = engine.PosTable(ctx, k, 2 * len(want))
        pt.insert(0, ss)
        pt.insert(1, ss)
        got, nmated = pt.mates(ss)
        pt.close()
        assert np.array_equal(got, want) and nmated == len(want)
    finally:
        ss.close()


def test_invalid_arguments_are_refused(ctx):
    from panagram_amd import engine
    for k, cap in ((0, 10), (33, 10), (-1, 10), (21, 0), (21, (1 << 32) + 1)):
        with pytest.raises(engine.PanagramHipError) as ei:
            engine.PosTable(ctx, k, cap)
        assert ei.value.code == PG_E_INVALID, (k, cap)
    ss = engine.SeqSet.from_host(ctx, [sr.ascii_of(sr.random_codes(100, 26))])
    pt = engine.PosTable(ctx, 21, 200)
    try:
        calls = [lambda: pt.mates(ss), lambda: pt.insert(2, ss), lambda: pt.insert(-1, ss)]
        for call in calls:
            with pytest.raises(engine.PanagramHipError) as ei:
                call()
            assert ei.value.code == PG_E_INVALID
        pt.insert(0, ss)
        with pytest.raises(engine.PanagramHipError) as ei:
            pt.insert(0, ss)  # a second time: every key would turn MULTI
        assert ei.value.code == PG_E_INVALID
        got, nmated = pt.mates(ss)  # B not inserted: no mate
        assert (got == NO).all() and nmated == 0
        for k in (0, 33):
            with pytest.raises(engine.PanagramHipError) as ei:
                engine.synteny_segments(ctx, k, ss, ss)
            assert ei.value.code == PG_E_INVALID
    finally:
        pt.close()
        ss.close()


# ---------------------------------------------------------------------------
# pg_synteny_segments
# ---------------------------------------------------------------------------
def _segments(ctx, a, b, k, cap=None):
    from panagram_amd import engine
    ssa, ssb = engine.SeqSet.from_host(ctx, a), engine.SeqSet.from_host(ctx, b)
    try:
        return engine.synteny_segments(ctx, k, ssa, ssb, cap)
    finally:
        ssa.close()
        ssb.close()


@pytest.mark.parametrize("d", [0.01, 0.05])
def test_segments_of_diverged_genomes(ctx, d):
    k = 21
    g = po.synth_genomes(2, [60000, 33333, 20011], d, 30)
    a, b = ([sr.ascii_of(c) for c in x] for x in g)
    want, mated = sr.segments(a, b, k)
    assert len(want) > 300
    got = _segments(ctx, a, b, k)
    _same_runs(got, want, d)
    assert got[5] == mated == int((want[:, 2] - want[:, 1]).sum())
    again = _segments(ctx, a, b, k)
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(got, again))
    # a first call whose arrays are too short is followed by one that fits
    small = _segments(ctx, a, b, k, cap=7)
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(got, small))


def test_segments_of_planted_rearrangements(ctx):
    k = sr.PLANTED_K
    x, y = sr.planted_contigs()
    a = [sr.ascii_of(x), sr.ascii_of(y)]
    b = [sr.ascii_of(c) for c in sr.planted_rearranged(x, y)]
    want, mated = sr.segments(a, b, k)
    assert want.tolist() == [[0, 0, 186, 0], [0, 200, 486, 1800], [0, 500, 886, 400], [1, 0, 86, 1200], [1, 100, 126, 1451],
                             [1, 140, 286, 1480], [1, 300, 686, 2400]]
    got = _segments(ctx, a, b, k)
    _same_runs(got, want)
    assert got[5] == mated
    # B against A, B = revcomp(A), a tandem duplication, SNPs, and the contigs of A adjacent in B
    _same_runs(_segments(ctx, b, a, k), sr.segments(b, a, k)[0], "B against A")
    r = [sr.ascii_of(sr.revcomp(y)), sr.ascii_of(sr.revcomp(x))]
    want = sr.segments(a, r, k)[0]
    assert want.tolist() == [[0, 0, 886, ((1600 - k) << 1) | 1], [1, 0, 686, ((700 - k) << 1) | 1]]
    _same_runs(_segments(ctx, a, r, k), want, "revcomp")
    dup = [sr.ascii_of(sr.plant_tandem_duplication(x, 300, 500)), sr.ascii_of(sr.plant_snps(y, [50, 51, 400, 699]))]
    _same_runs(_segments(ctx, a, dup, k), sr.segments(a, dup, k)[0], "duplication and SNPs")
    s = np.concatenate([x, y])
    halves = [sr.ascii_of(s[:500 + k - 1]), sr.ascii_of(s[500:])]
    want = sr.segments(halves, [sr.ascii_of(s)], k)[0]
    assert want.tolist() == [[0, 0, 500, 0], [1, 0, 1600 - k + 1 - 500, 1000]]
    _same_runs(_segments(ctx, halves, [sr.ascii_of(s)], k), want, "adjacent contigs")
    # nothing shared, and a side without k-mers
    got = _segments(ctx, a, [sr.ascii_of(sr.random_codes(500, 31))], k)
    assert len(got[0]) == 0 and got[4].tolist() == [0, 0] and got[5] == 0
    got = _segments(ctx, a, [b"ACGT"], k)
    assert len(got[0]) == 0 and got[5] == 0
