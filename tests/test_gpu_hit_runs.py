"""GPU: k_hit_runs (panagram_amd/csrc/pg_locate.hip) through PosTable.hit_runs and PosTable.locate against the numpy model
(tests/locate_ref.py), array for array — order included — on the crafted queries and genome that hold every edge of the kernel
(tests/test_locate_cpu.py proves that they do), on the small cases at k = 6, 31 and 32 and on 1025 queries."""
import ctypes as C

import numpy as np
import pytest

from tests import locate_ref as lr

pytestmark = pytest.mark.gpu

NO = lr.NO_MATE
PG_E_INVALID, PG_E_CAPACITY = -1, -4


class Case:
    """queries and a genome on the GPU with the queries inserted as side 1, and the model's arrays of them"""

    def __init__(self, ctx, k, q, g, capacity=None):
        from panagram_amd import engine
        self.k, self.q, self.g = k, q, g
        self.qs, self.gs = engine.SeqSet.from_host(ctx, q), engine.SeqSet.from_host(ctx, g)
        self.pt = engine.PosTable(ctx, k, max(1, self.qs.total_kmers(k)) if capacity is None else capacity)
        self.pt.insert(1, self.qs)
        self.runs, self.per, self.hits = lr.hit_runs(g, q, k)

    def close(self):
        self.pt.close()
        self.qs.close()
        self.gs.close()


@pytest.fixture(scope="module")
def crafted(ctx):
    c = lr.crafted()
    case = Case(ctx, c["k"], c["q"], c["g"])
    case.params = c["params"]
    yield case
    case.close()


def _same_runs(got, runs, per, hits, tag=""):
    rc, rs, re_, rh, gper, ghits = got[:6]
    assert len(rc) == len(runs), (tag, len(rc), len(runs))
    assert np.array_equal(np.stack([rc, rs, re_, rh], axis=1).astype(np.int64), runs), tag
    assert np.array_equal(gper.astype(np.int64), per) and np.array_equal(ghits.astype(np.int64), hits), tag


def _same_blocks(got, want, tag=""):
    blk, per, nhits, nruns = want
    assert np.array_equal(np.stack(got[:8], axis=1).astype(np.int64), blk), tag
    assert np.array_equal(got[8].astype(np.int64), per) and (got[9], got[10]) == (nhits, nruns), tag


def test_hit_runs_on_crafted(crafted):
    got = crafted.pt.hit_runs(crafted.gs)
    _same_runs(got, crafted.runs, crafted.per, crafted.hits)
    again = crafted.pt.hit_runs(crafted.gs)  # the same on every call
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again))


def test_locate_on_crafted(crafted):
    want = lr.blocks(crafted.g, crafted.q, crafted.k, **crafted.params)
    got = crafted.pt.locate(crafted.gs, crafted.qs, **crafted.params)
    _same_blocks(got, want)
    again = crafted.pt.locate(crafted.gs, crafted.qs, **crafted.params, cap=3)  # (too few: a second call inside)
    assert all(np.array_equal(x, y) for x, y in zip(got, again))
    for params in (dict(min_run=1, max_gap=1, max_shift=0), dict(min_run=12, max_gap=25, max_shift=4), dict(min_run=2, max_gap=26, max_shift=5)):
        _same_blocks(crafted.pt.locate(crafted.gs, crafted.qs, **params), lr.blocks(crafted.g, crafted.q, crafted.k, **params), params)


def test_the_queries_against_their_own_table_give_unique(crafted):
    got = crafted.pt.hit_runs(crafted.qs)
    want = lr.unique_per_query(crafted.q, crafted.k)
    assert np.array_equal(got[5].astype(np.int64), want)
    _same_runs(got, *lr.hit_runs(crafted.q, crafted.q, crafted.k))


@pytest.mark.parametrize("name", ["k6", "k31", "k32", "1025 queries", "64 slots"])
def test_small_cases(ctx, name):
    """"64 slots": eight sets of 32 keys in a table made for 32 — the walk passes the table's end (lr.wrap_cases)"""
    for k, q, g in (lr.wrap_cases() if name == "64 slots" else [lr.small_cases()[name]]):
        case = Case(ctx, k, q, g, capacity=32 if name == "64 slots" else None)
        try:
            _same_runs(case.pt.hit_runs(case.gs), case.runs, case.per, case.hits, name)
            _same_blocks(case.pt.locate(case.gs, case.qs), lr.blocks(g, q, k), name)
            assert np.array_equal(case.pt.hit_runs(case.qs)[5].astype(np.int64), lr.unique_per_query(q, k)), name
        finally:
            case.close()


def test_capacity_protocol(crafted):
    total = len(crafted.runs)
    for cap in (0, total - 1):
        *arrs, per, hits, got_total, nhits = crafted.pt.hit_runs(crafted.gs, cap=cap)
        assert got_total == total and nhits == crafted.hits.sum(), cap
        assert np.array_equal(per.astype(np.int64), crafted.per) and np.array_equal(hits.astype(np.int64), crafted.hits), cap
        assert all((a == NO).all() for a in arrs), cap  # nothing is written
    *arrs, per, hits, got_total, nhits = crafted.pt.hit_runs(crafted.gs, cap=total)
    assert got_total == total
    _same_runs((*arrs, per, hits), crafted.runs, crafted.per, crafted.hits, "cap = total")
    # hits_per_contig may be NULL; the arrays may be NULL at cap = 0
    lib, n = crafted.pt._lib, len(crafted.g)
    per, tot, nh = np.zeros(n, np.uint64), C.c_uint64(), C.c_uint64()
    assert lib.pg_postable_hit_runs(crafted.pt._h, crafted.gs._h, 0, None, None, None, None, per.ctypes.data, None, C.byref(tot), C.byref(nh)) == 0
    assert tot.value == total and nh.value == crafted.hits.sum() and np.array_equal(per.astype(np.int64), crafted.per)
    # the blocks: nothing written below the total
    want = lr.blocks(crafted.g, crafted.q, crafted.k, **crafted.params)
    nb = len(want[0])
    for cap in (0, nb - 1, nb):
        arrs = [np.full(cap, NO, np.uint32) for _ in range(8)]
        per, tot, nh, nr = np.zeros(n, np.uint64), C.c_uint64(), C.c_uint64(), C.c_uint64()
        p = crafted.params
        rc = lib.pg_postable_locate(crafted.pt._h, crafted.gs._h, crafted.qs._h, p["min_run"], p["max_gap"], p["max_shift"], cap,
                                    *[a.ctypes.data if cap else None for a in arrs], per.ctypes.data, C.byref(tot), C.byref(nh), C.byref(nr))
        assert rc == 0 and (tot.value, nh.value, nr.value) == (nb, want[2], want[3]) and np.array_equal(per.astype(np.int64), want[1]), cap
        if cap < nb:
            assert all((a == NO).all() for a in arrs), cap
        else:
            assert np.array_equal(np.stack(arrs, axis=1).astype(np.int64), want[0])


def test_one_table_serves_three_genomes_in_turn(ctx, crafted):
    from panagram_amd import engine
    g, q, k = crafted.g, crafted.q, crafted.k
    others = [[g[6], g[4], g[1]], [lr.revcomp(g[1]), b"", g[0][3000:9000]], g]
    for i, contigs in enumerate(others):
        ss = engine.SeqSet.from_host(ctx, contigs)
        try:
            _same_runs(crafted.pt.hit_runs(ss), *lr.hit_runs(contigs, q, k), i)
            _same_blocks(crafted.pt.locate(ss, crafted.qs, **crafted.params), lr.blocks(contigs, q, k, **crafted.params), i)
        finally:
            ss.close()


def test_a_genome_without_positions_and_queries_without(ctx):
    from panagram_amd import engine
    k = 21
    case = Case(ctx, k, [b"ACGT", b""], [b"ACGTACGTAC", b"", b"A" * 40])
    try:
        got = case.pt.hit_runs(case.gs)
        assert all(len(a) == 0 for a in got[:4]) and not got[4].any() and not got[5].any()
        got = case.pt.locate(case.gs, case.qs)
        assert all(len(a) == 0 for a in got[:8]) and got[9:] == (0, 0)
        none = engine.SeqSet.from_host(ctx, [])
        try:
            assert len(case.pt.hit_runs(none)[0]) == 0 and case.pt.locate(none, case.qs)[9:] == (0, 0)
        finally:
            none.close()
    finally:
        case.close()


def _refused(call, code):
    from panagram_amd import engine
    with pytest.raises(engine.PanagramHipError) as ei:
        call()
    assert ei.value.code == code


def test_invalid_calls_are_refused_before_anything_runs(ctx, crafted):
    from panagram_amd import engine
    k = crafted.k
    pt = engine.PosTable(ctx, k, crafted.gs.total_kmers(k))
    other_ctx = engine.Context(0)
    foreign = engine.SeqSet.from_host(other_ctx, [crafted.g[4]])
    fewer = engine.SeqSet.from_host(ctx, crafted.q[:-1])           # other contigs, other bases
    shuffled = engine.SeqSet.from_host(ctx, crafted.q[:-2] + [crafted.q[-2] + crafted.q[-1][:5], crafted.q[-1][5:]])  # same contigs and bases: taken
    try:
        # side 1 not inserted — inserting side 0 does not help
        _refused(lambda: pt.hit_runs(crafted.gs), PG_E_INVALID)
        pt.insert(0, crafted.gs)
        _refused(lambda: pt.hit_runs(crafted.gs), PG_E_INVALID)
        _refused(lambda: pt.locate(crafted.gs, crafted.qs), PG_E_INVALID)
        # a foreign context, on either argument
        _refused(lambda: crafted.pt.hit_runs(foreign), PG_E_INVALID)
        _refused(lambda: crafted.pt.locate(foreign, crafted.qs), PG_E_INVALID)
        _refused(lambda: crafted.pt.locate(crafted.gs, foreign), PG_E_INVALID)
        # seqsQ is not the set inserted as side 1
        _refused(lambda: crafted.pt.locate(crafted.gs, fewer), PG_E_INVALID)
        _refused(lambda: crafted.pt.locate(crafted.gs, crafted.gs), PG_E_INVALID)
        crafted.pt.locate(crafted.gs, shuffled)  # (the table remembers bases and contigs, no more)
        # the parameters, as pg_run_blocks
        for bad in (dict(min_run=0), dict(max_gap=0), dict(max_gap=1 << 31), dict(max_shift=1 << 31)):
            _refused(lambda: crafted.pt.locate(crafted.gs, crafted.qs, **bad), PG_E_INVALID)
        # NULL arguments; a refused call leaves the counts as they were
        lib, n = crafted.pt._lib, len(crafted.g)
        per, tot, nh, nr = np.full(n, 77, np.uint64), C.c_uint64(77), C.c_uint64(77), C.c_uint64(77)
        assert lib.pg_postable_hit_runs(crafted.pt._h, crafted.gs._h, 0, None, None, None, None, per.ctypes.data, None, None, C.byref(nh)) == PG_E_INVALID
        assert lib.pg_postable_hit_runs(crafted.pt._h, crafted.gs._h, 5, None, None, None, None, per.ctypes.data, None, C.byref(tot), C.byref(nh)) == PG_E_INVALID
        assert lib.pg_postable_hit_runs(None, crafted.gs._h, 0, None, None, None, None, per.ctypes.data, None, C.byref(tot), C.byref(nh)) == PG_E_INVALID
        assert lib.pg_postable_locate(crafted.pt._h, crafted.gs._h, fewer._h, 1, 1000, 100, 0, *[None] * 8, per.ctypes.data, C.byref(tot), C.byref(nh),
                                      C.byref(nr)) == PG_E_INVALID
        assert lib.pg_postable_locate(crafted.pt._h, crafted.gs._h, crafted.qs._h, 1, 1000, 100, 0, *[None] * 8, per.ctypes.data, None, C.byref(nh),
                                      C.byref(nr)) == PG_E_INVALID
        assert (per == 77).all() and (tot.value, nh.value, nr.value) == (77, 77, 77)
        assert lib.pg_locate_last_timing(None) == PG_E_INVALID
    finally:
        pt.close()
        for s in (foreign, fewer, shuffled):
            s.close()
        other_ctx.close()


def test_an_overflowed_table_answers_capacity(ctx, crafted):
    from panagram_amd import engine
    pt = engine.PosTable(ctx, crafted.k, 8)  # 16 slots for thousands of keys
    try:
        _refused(lambda: pt.insert(1, crafted.qs), PG_E_CAPACITY)
        _refused(lambda: pt.hit_runs(crafted.gs), PG_E_CAPACITY)
        _refused(lambda: pt.locate(crafted.gs, crafted.qs), PG_E_CAPACITY)
    finally:
        pt.close()
    # a table filled to the brim answers as a roomy one: capacity = the distinct keys, half the slots
    tight = Case(ctx, crafted.k, crafted.q, crafted.g, capacity=len(np.unique(lr.sr.side_kmers(crafted.q, crafted.k)[0])))
    try:
        _same_runs(tight.pt.hit_runs(tight.gs), crafted.runs, crafted.per, crafted.hits, "tight")
    finally:
        tight.close()


def test_one_contig_holds_2_32_minus_1_positions_and_no_more(ctx):
    """the limit of the streamed side is one contig's positions, not the total: a contig of 2^32 - 1 k-mer positions of A only (a
    sequence set is all A until something is loaded), counted without emitting — every position hits the one k-mer of the query,
    no position continues its predecessor (the word does not advance), so runs = hits = 2^32 - 1, the last chunk starting at
    2^32 - 4096: first position + 4096 does not fit 32 bits.  One position more is refused."""
    from panagram_amd import engine
    k = 21
    qs = engine.SeqSet.from_host(ctx, [b"A" * k, b"ACGTTGCATGCATGCCGTAGCATGGT"])
    pt = engine.PosTable(ctx, k, 64)
    pt.insert(1, qs)
    big = engine.SeqSet(ctx, [(1 << 32) - 1 + k - 1, 30])
    try:
        *arrs, per, hits, total, nhits = pt.hit_runs(big, cap=0)
        n = (1 << 32) - 1
        assert (total, nhits) == (n + 10, n + 10) and per.tolist() == [n, 10] and hits.tolist() == [n, 10]
    finally:
        big.close()
    more = engine.SeqSet(ctx, [30, (1 << 32) + k - 1])
    try:
        _refused(lambda: pt.hit_runs(more, cap=0), PG_E_INVALID)
        _refused(lambda: pt.locate(more, qs), PG_E_INVALID)
    finally:
        more.close()
        pt.close()
        qs.close()


def test_last_timing(crafted):
    from panagram_amd import engine
    crafted.pt.locate(crafted.gs, crafted.qs, **crafted.params)
    t = engine.locate_last_timing()
    assert list(t) == ["hits_count_ms", "hits_emit_ms", "blocks_count_ms", "blocks_emit_ms"] and all(v > 0 for v in t.values())
    crafted.pt.hit_runs(crafted.gs, cap=0)
    t = engine.locate_last_timing()
    assert t["hits_count_ms"] > 0 and t["hits_emit_ms"] == t["blocks_count_ms"] == t["blocks_emit_ms"] == 0
