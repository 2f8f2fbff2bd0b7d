"""GPU: the allele kernels (panagram_amd/csrc/pg_genotype.hip) through engine.CopyTable against the model (tests/genotype_ref.py),
exactly, at k = 6, 21, 31 and 32 (32 uses the key's whole word): insert_ranges' newly claimed keys over two successive calls, and
allele_support's windows, informative and seen windows and 64-bit depth sums on the crafted set — alleles of one and of no base,
ranges clipped at a contig's ends, contigs of fewer than and of exactly k bases, non-ACGT bases in and beside the allele, piece and
block edges, keys that are never informative, a range that was never inserted, and a homopolymer whose one counter passes 65 535."""
import ctypes as C

import numpy as np
import pytest

from tests import genotype_ref as gr

pytestmark = pytest.mark.gpu

PG_E_INVALID, PG_E_CAPACITY = -1, -4
KS = (6, 21, 31, 32)


def _cols(ranges):
    r = np.asarray(ranges, np.int64).reshape(-1, 3)
    return r[:, 0].astype(np.uint32), r[:, 1].astype(np.uint64), r[:, 2].astype(np.uint64)


class _Crafted:
    """the crafted set on the GPU: the sequence set, a table with both inserts done and the three planes counted"""

    def __init__(self, ctx, k):
        from panagram_amd import engine
        self.case = gr.crafted(k)
        self.model, self.distinct, self.hits = gr.crafted_model(self.case, k)
        self.ss = engine.SeqSet.from_host(ctx, self.case["seqs"])
        self.table = engine.CopyTable(ctx, k, 20000, 3)
        self.got_distinct = [self.table.insert_ranges(self.ss, *_cols(rs)) for rs in self.case["inserted"]]
        self.got_hits = []
        for g, contigs in enumerate(self.case["genomes"]):
            gs = engine.SeqSet.from_host(ctx, contigs)
            try:
                self.got_hits.append(self.table.count(g, gs))
            finally:
                gs.close()

    def close(self):
        self.table.close()
        self.ss.close()


@pytest.fixture(scope="module")
def crafted21(ctx):
    c = _Crafted(ctx, 21)
    yield c
    c.close()


@pytest.mark.parametrize("k", KS)
def test_allele_support_equals_the_model(ctx, k):
    from panagram_amd import engine
    c = _Crafted(ctx, k)
    try:
        # insert_ranges: the keys each of two successive calls added; the planes' hits
        assert c.got_distinct == c.distinct and c.distinct[0] > 0 and c.distinct[1] > 0
        assert c.got_hits == c.hits
        names = list(c.case["ranges"])
        ranges = [c.case["ranges"][n] for n in names]
        for own, other, min_count in ((0, 1, gr.MIN_COUNT), (1, 0, gr.MIN_COUNT), (0, 1, 1), (0, 1, gr.MIN_COUNT + 1), (0, 2, 1)):
            got = c.table.allele_support(c.ss, *_cols(ranges), own, other, 2, min_count)
            want = c.model.support(c.case["seqs"], ranges, own, other, 2, min_count)
            assert all(x.dtype == np.uint64 and len(x) == len(ranges) for x in got)
            for what, g, w in zip(("windows", "inf", "seen", "depth"), got, want):
                bad = [(names[i], int(g[i]), w[i]) for i in range(len(names)) if int(g[i]) != w[i]]
                assert not bad, (k, own, other, min_count, what, bad[:5])
        ms = engine.genotype_last_timing()
        assert list(ms) == ["insert_ms", "support_ms"] and ms["insert_ms"] > 0 and ms["support_ms"] > 0
        assert engine.CopyTable.genotype_last_timing() == ms
        # what the crafted set holds, by construction (the model said the same above)
        got = dict(zip(names, zip(*(x.tolist() for x in c.table.allele_support(c.ss, *_cols(ranges), 0, 1, 2, gr.MIN_COUNT)))))
        for n in ("junction_at_0", "junction_at_L", "short_contig", "short_junction", "n_alone"):
            assert got[n] == (0, 0, 0, 0), n
        assert got["one_base"][0] == k and got["junction"][0] == k - 1 and got["first_base"][0] == 1 and got["last_base"][0] == 1
        assert got["first_window"][0] == 5 and got["last_window"][0] == 2 and got["exact_contig"][0] == 1 and got["exact_junction"][0] == 1
        assert got["n_inside"][0] == 10 + k - 1 - k and got["n_beside"][0] == k - 1  # (the k windows that hold base 100 do not exist)
        for w in (63, 64, 65, 257, 4097):
            assert got[f"windows_{w}"][0] == w
        assert got["never"][0] == 100 + k - 1 and got["in_neither"][0] == 100 + k - 1
        run = gr.LONG_RUN - k + 1  # the homopolymer's windows, all of one key: once in own, `run` times in the sample
        assert got["long_run"] == (run, run, run, run * run) and run * run > 1 << 32 and run > 65535
        assert got["long_run_junction"] == (k - 1, k - 1, k - 1, (k - 1) * run)
        if k >= 21:  # (random k-mers are distinct: the crafted depths hold for every window)
            assert got["one_base"] == (k, k, k, k * gr.MIN_COUNT) and got["junction"][1:3] == (k - 1, k - 1)
            assert got["twice_in_own"][1] == 0 and got["own_and_other"][1] == 0 and got["in_neither"][1] == 0 and got["never"][1] == 0
            assert got["depth_0"][1:] == (30 + k - 1, 0, 0)
            assert got["depth_below"][1:] == (30 + k - 1, 0, (30 + k - 1) * (gr.MIN_COUNT - 1))
            assert got["depth_at"][1:] == (30 + k - 1, 30 + k - 1, (30 + k - 1) * gr.MIN_COUNT)
            assert 0 < got["depth_across"][2] < got["depth_across"][1]
            assert got["shares_a"][1] == k and got["shares_b"][1] == k + 1
    finally:
        c.close()


def test_no_range_and_3000_ranges_in_one_call(ctx, crafted21):
    c = crafted21
    empty = c.table.allele_support(c.ss, [], [], [], 0, 1, 2, 1)
    assert [len(x) for x in empty] == [0] * 4 and c.table.insert_ranges(c.ss, [], [], []) == 0
    many = gr.many_ranges()
    assert len(many) == 3000
    got = c.table.allele_support(c.ss, *_cols(many), 0, 1, 2, gr.MIN_COUNT)
    want = c.model.support(c.case["seqs"], many, 0, 1, 2, gr.MIN_COUNT)
    for g, w in zip(got, want):
        assert g.tolist() == w
    assert sum(want[1]) > 10000 and 0 < sum(want[2]) < sum(want[1])
    # their keys into a table of their own: distinct is the model's, and a second insert adds none
    from panagram_amd import engine
    t = engine.CopyTable(ctx, 21, 20000, 2)
    try:
        m = gr.Table(21, 2)
        assert t.insert_ranges(c.ss, *_cols(many)) == m.insert_ranges(c.case["seqs"], many) > 5000
        assert t.insert_ranges(c.ss, *_cols(many[:100])) == 0
    finally:
        t.close()


def test_invalid_arguments_launch_nothing(ctx, crafted21):
    from panagram_amd import engine
    c, lib = crafted21, ctx._lib
    L = len(c.case["seqs"][0])
    ranges = [c.case["ranges"][n] for n in ("one_base", "windows_257", "long_run")]
    before = [x.tolist() for x in c.table.allele_support(c.ss, *_cols(ranges), 0, 1, 2, gr.MIN_COUNT)]
    ms = engine.genotype_last_timing()
    other_ctx = engine.Context(0)
    foreign = engine.SeqSet.from_host(other_ctx, [b"ACGT" * 50])
    cg, st, ln = (np.array(x) for x in _cols([(0, 10, 5)]))
    out = [np.zeros(1, np.uint64) for _ in range(4)]
    n = C.c_uint64()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    nseq = len(c.case["seqs"])

    def support(ct=None, ss=None, count=1, contig=cg, start=st, length=ln, own=0, other=1, sample=2, min_count=1, outs=None):
        outs = out if outs is None else outs
        return lib.pg_copytable_allele_support(c.table._h if ct is None else ct, c.ss._h if ss is None else ss, count, p(contig), p(start),
                                               p(length), own, other, sample, min_count, *[None if o is None else p(o) for o in outs])

    def insert(ct=None, ss=None, count=1, contig=cg, start=st, length=ln, distinct=n):
        return lib.pg_copytable_insert_ranges(c.table._h if ct is None else ct, c.ss._h if ss is None else ss, count, p(contig), p(start),
                                              p(length), None if distinct is None else C.byref(distinct))
    u32, u64 = (lambda v: np.array([v], np.uint32)), (lambda v: np.array([v], np.uint64))
    # 2^31 - 1 pieces and one more: the homopolymer's whole range, 1 094 pieces, often enough
    per = (gr.LONG_RUN - 21 + 1 + 63) // 64
    reps = (1 << 31) // per + 1
    big = (np.full(reps, 4, np.uint32), np.zeros(reps, np.uint64), np.full(reps, gr.LONG_RUN, np.uint64))
    big_out = [np.zeros(reps, np.uint64) for _ in range(4)]
    try:
        calls = [
            lambda: lib.pg_copytable_allele_support(None, c.ss._h, 1, p(cg), p(st), p(ln), 0, 1, 2, 1, *[p(o) for o in out]),
            lambda: lib.pg_copytable_allele_support(c.table._h, None, 1, p(cg), p(st), p(ln), 0, 1, 2, 1, *[p(o) for o in out]),
            lambda: lib.pg_copytable_allele_support(c.table._h, c.ss._h, 1, None, p(st), p(ln), 0, 1, 2, 1, *[p(o) for o in out]),
            lambda: lib.pg_copytable_allele_support(c.table._h, c.ss._h, 1, p(cg), None, p(ln), 0, 1, 2, 1, *[p(o) for o in out]),
            lambda: lib.pg_copytable_allele_support(c.table._h, c.ss._h, 1, p(cg), p(st), None, 0, 1, 2, 1, *[p(o) for o in out]),
            lambda: support(outs=[None] + out[1:]), lambda: support(outs=out[:1] + [None] + out[2:]),
            lambda: support(outs=out[:2] + [None] + out[3:]), lambda: support(outs=out[:3] + [None]),
            lambda: support(ss=foreign._h),
            lambda: support(contig=u32(nseq)), lambda: support(start=u64(L - 4)), lambda: support(start=u64(L + 1), length=u64(0)),
            lambda: support(start=u64(1), length=u64((1 << 64) - 1)),
            lambda: support(own=3), lambda: support(other=3), lambda: support(sample=3), lambda: support(min_count=0),
            lambda: support(own=1, other=1),
            lambda: support(count=reps, contig=big[0], start=big[1], length=big[2], outs=big_out),
            lambda: lib.pg_copytable_insert_ranges(None, c.ss._h, 1, p(cg), p(st), p(ln), C.byref(n)),
            lambda: lib.pg_copytable_insert_ranges(c.table._h, None, 1, p(cg), p(st), p(ln), C.byref(n)),
            lambda: lib.pg_copytable_insert_ranges(c.table._h, c.ss._h, 1, None, p(st), p(ln), C.byref(n)),
            lambda: lib.pg_copytable_insert_ranges(c.table._h, c.ss._h, 1, p(cg), None, p(ln), C.byref(n)),
            lambda: lib.pg_copytable_insert_ranges(c.table._h, c.ss._h, 1, p(cg), p(st), None, C.byref(n)),
            lambda: insert(distinct=None), lambda: insert(ss=foreign._h), lambda: insert(contig=u32(nseq)), lambda: insert(start=u64(L - 4)),
            lambda: insert(start=u64(1), length=u64((1 << 64) - 1)),
            lambda: insert(count=reps, contig=big[0], start=big[1], length=big[2]),
            lambda: lib.pg_genotype_last_timing(None),
        ]
        for i, call in enumerate(calls):
            assert call() == PG_E_INVALID, i
            assert lib.pg_last_error()
        # nothing was launched: the timings of the last launches stand, the table answers as before, and holds no new key
        assert engine.genotype_last_timing() == ms
        assert all(not o.any() for o in out) and not big_out[0].any()
        # n == 0 with NULL arrays is no error
        assert lib.pg_copytable_allele_support(c.table._h, c.ss._h, 0, None, None, None, 0, 1, 2, 1, None, None, None, None) == 0
        assert lib.pg_copytable_insert_ranges(c.table._h, c.ss._h, 0, None, None, None, C.byref(n)) == 0 and n.value == 0
        assert [x.tolist() for x in c.table.allele_support(c.ss, *_cols(ranges), 0, 1, 2, gr.MIN_COUNT)] == before
        assert c.table.insert_ranges(c.ss, *_cols(ranges)) == 0
        with pytest.raises(ValueError):
            c.table.allele_support(c.ss, [0], [1], [1], 0, 1, 2, -1)
        with pytest.raises(ValueError):
            c.table.insert_ranges(c.ss, [0, 0], [1], [1])
    finally:
        foreign.close()
        other_ctx.close()


def test_a_table_made_too_small_stays_full(ctx, crafted21):
    from panagram_amd import engine
    c = crafted21
    t = engine.CopyTable(ctx, 21, 4, 3)  # 8 slots
    try:
        with pytest.raises(engine.PanagramHipError) as ei:
            t.insert_ranges(c.ss, [0], [100], [3000])
        assert ei.value.code == PG_E_CAPACITY
        for call in (lambda: t.insert_ranges(c.ss, [0], [100], [1]), lambda: t.allele_support(c.ss, [0], [100], [1], 0, 1, 2, 1),
                     lambda: t.insert_ranges(c.ss, [], [], [])):
            with pytest.raises(engine.PanagramHipError) as ei:
                call()
            assert ei.value.code == PG_E_CAPACITY  # sticky
        with pytest.raises(engine.PanagramHipError) as ei:
            t.allele_support(c.ss, [0], [100], [1], 0, 0, 2, 1)
        assert ei.value.code == PG_E_INVALID  # (the arguments are judged first)
    finally:
        t.close()
