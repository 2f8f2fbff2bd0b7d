"""GPU: k_sample_agree (panagram_amd/csrc/pg_place.hip) on rows PLANTED into a rows container (tests/rows_craft.py: dense rows, the
bits past N set, every byte that is no row byte 0xFF), an anchor seqset and a count table counted from crafted reads
(tests/place_ref.py: agree_case).  valid, held, col and both are exactly the numpy model's.

Which kernel runs for which N: N <= 128 k_sample_agree<4, 1> (the row's words in registers), N <= 256 <0, 1>, beyond <0, 2> (two
columns per thread); a wave takes 64 rows, a tile 256, a workgroup's chunk engine.PLACE_CHUNK rows from its window's first."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import place_ref as pr
from tests import rows_craft as rc

pytestmark = pytest.mark.gpu

PG_E_INVALID = -1


@functools.lru_cache(maxsize=None)
def _case(k):
    case = pr.agree_case(k)
    case["depths"] = pr.sample_depths(case["anchor"], pr.joined_reads(case["reads"]), k)
    return case


class _Setup:
    """anchor seqset, reads counted into plane 0 of a count table (through from_fastq), and a planted rows container"""

    def __init__(self, ctx, k, n, table_k=None):
        from panagram_amd import engine
        self.case = case = _case(k)
        self.n, self.k = n, k
        self.rows = pr.agree_rows(case["nkmers"], n, seed=n)
        self.anchor = engine.SeqSet.from_host(ctx, case["anchor"])
        self.table = self.res = None
        try:
            self.table = engine.CopyTable(ctx, k if table_k is None else table_k, sum(len(a) for a in case["anchor"]), 1)
            self.table.insert(self.anchor)
            reads, nreads, used = engine.SeqSet.from_fastq(ctx, pr.fastq_text(case["reads"]))
            try:
                assert nreads == len(case["reads"])
                self.table.count(0, reads)
            finally:
                reads.close()
            self.res = rc.container(ctx, k, n, case["nkmers"], colsums=False)
            rc.plant(self.res, self.rows, poison=0xFF)
            self.res.rows_epilogue()  # (a rows container is read once its statistics have been enqueued)
        except Exception:
            self.close()
            raise

    def check(self, min_count, windows=None, tag=""):
        c, s, e = self.case["windows"] if windows is None else windows
        got = self.table.sample_agree(0, min_count, self.anchor, self.res, c, s, e)
        want = pr.agree(self.case["depths"], self.rows, self.n, min_count, c, s, e)
        for g, w, name in zip(got, want, ("valid", "held", "col", "both")):
            assert g.dtype == np.uint64 and g.shape == w.shape, (tag, name)
            bad = np.argwhere(g != w)
            assert not len(bad), f"k={self.k} N={self.n} min_count={min_count} {tag}: {name}{bad[0].tolist()} = {g[tuple(bad[0])]}, " \
                                 f"the model {w[tuple(bad[0])]} ({len(bad)} differ)"
        return got

    def close(self):
        for x in (self.res, self.table, self.anchor):
            if x is not None:
                x.close()


@pytest.mark.parametrize("n", pr.AGREE_N)
def test_every_row_width(ctx, n):
    s = _Setup(ctx, 21, n)
    try:
        valid, held, col, both = s.check(2)
        c, st, en = s.case["windows"]
        empty = st == en
        assert empty.any() and not valid[empty].any() and not col[empty].any()
        assert held.sum() > 1000 and (held <= valid).all() and held.sum() < valid.sum() and (both <= col).all() and both.sum() > 100 * n
    finally:
        s.close()


@pytest.mark.parametrize("k", pr.AGREE_K)
def test_every_k_and_min_count_on_one_table(ctx, k):
    s = _Setup(ctx, k, 9)
    try:
        held = [int(s.check(m, tag="min_count")[1].sum()) for m in pr.AGREE_MIN_COUNTS]
        assert held[0] >= held[1] >= held[2] > 0 and held[0] > held[2]  # (rows of depth 1, and of depth 2 and 4, fall out)
        big = s.check(pr.DEEP)[1]
        assert big.sum() >= 1 and s.check(pr.DEEP + 1000)[1].sum() == 0
        # the planted rows one by one: depth min_count - 1 is not held, min_count is
        if k > 6:
            sp = s.case["special"]
            one = lambda name: (np.array([0], np.uint32), np.array([sp[name][1]], np.uint64), np.array([sp[name][1] + 1], np.uint64))
            for name, depth in (("d0", 0), ("d1", 1), ("d2", 2), ("d3", 4), ("d4", 5), ("d5", pr.DEEP), ("rc_only", 3), ("never", 0)):
                for m in pr.AGREE_MIN_COUNTS:
                    valid, h, _, _ = s.check(m, one(name), name)
                    assert valid[0] == 1 and h[0] == int(depth >= m), (name, m)
            for name in ("dup", "dup2", "dup_rc"):  # one key at three rows, the third on the other strand: the same answer
                assert s.check(2, one(name), name)[1][0] == 1
    finally:
        s.close()


def test_windows_given_one_at_a_time_and_none(ctx):
    s = _Setup(ctx, 21, 33)
    try:
        c, st, en = s.case["windows"]
        for i in range(len(c)):
            s.check(2, (c[i:i + 1], st[i:i + 1], en[i:i + 1]), f"window {i}")
        got = s.table.sample_agree(0, 2, s.anchor, s.res, [], [], [])
        assert got[0].shape == (0,) and got[2].shape == (0, 33)
    finally:
        s.close()


def _raw(s, plane, min_count, c, st, en, table=None, anchor=None):
    c, st, en = np.ascontiguousarray(c, np.uint32), np.ascontiguousarray(st, np.uint64), np.ascontiguousarray(en, np.uint64)
    n = len(c)
    out = [np.full(n, 77, np.uint64), np.full(n, 77, np.uint64), np.full((n, s.n), 77, np.uint64), np.full((n, s.n), 77, np.uint64)]
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    code = s.res._lib.pg_copytable_sample_agree((table or s.table)._h, plane, min_count, (anchor or s.anchor)._h, s.res._h, n, vp(c), vp(st),
                                                vp(en), *[vp(o) for o in out])
    return code, out


def test_refusals_leave_the_outputs_alone(ctx):
    from panagram_amd import engine
    s = _Setup(ctx, 21, 12)
    nk = s.case["nkmers"]
    other_k = engine.CopyTable(ctx, 20, 1000, 1)
    wrong = engine.SeqSet.from_host(ctx, [s.case["anchor"][0] + b"A", s.case["anchor"][1], s.case["anchor"][2]])
    fewer = engine.SeqSet.from_host(ctx, s.case["anchor"][:2])
    wide = rc.container(ctx, 21, 513, nk, colsums=False)
    try:
        ok = ([0], [0], [100])
        for kw, args, msg in [
                ({}, (0, 0, *ok), "min_count must be >= 1"),
                ({}, (1, 2, *ok), "plane 1 of 1"),
                ({}, (0, 2, [0], [0], [nk[0] + 1]), f"window 0: sampled row {nk[0]} (x 1) past the {nk[0]} rows of contig 0"),
                ({}, (0, 2, [1], [0], [1]), "window 0: sampled row 0 (x 1) past the 0 rows of contig 1"),
                ({}, (0, 2, [3], [0], [1]), "window 0: contig 3 out of range"),
                ({}, (0, 2, [0], [5], [4]), "window 0: start 5 past end 4"),
                ({"anchor": wrong}, (0, 2, *ok), f"contig 0 has {nk[0]} rows, its {len(s.case['anchor'][0]) + 1} bases hold {nk[0] + 1} k-mers"),
                ({"anchor": fewer}, (0, 2, *ok), "the anchor has 2 contigs, the rows 3"),
                ({"table": other_k}, (0, 2, *ok), "rows of k = 21, a table of k = 20")]:
            code, out = _raw(s, *args, **kw)
            err = s.res._lib.pg_last_error().decode()
            assert code == PG_E_INVALID and err.endswith(msg), (err, msg)
            assert all((o == 77).all() for o in out), msg
            s.check(2, tag="after a refusal")
        with pytest.raises(engine.PanagramHipError, match="1 to 512") as ei:
            s.table.sample_agree(0, 2, s.anchor, wide, *ok)
        assert ei.value.code == PG_E_INVALID
        code, _ = _raw(s, 0, 2, [0], [0], [1])
        assert code == 0
    finally:
        for x in (wide, fewer, wrong, other_k):
            x.close()
        s.close()
