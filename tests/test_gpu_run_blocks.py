"""GPU: k_run_blocks (panagram_amd/csrc/pg_blocks.hip) through pg_run_blocks on the crafted run list of tests/blocks_ref.py —
no hashing involved — against the numpy model, exactly, order included: a wave takes 64 runs, a tile 256, a workgroup's chunk
4096, and the chunks' edges are stitched on the host.  Then the capacity protocol, every invalid argument, the empty list, and
the identity that ties the blocks to the runs."""
import ctypes as C

import numpy as np
import pytest

from tests import blocks_ref as br
from tests import synteny_ref as sr

pytestmark = pytest.mark.gpu

NO = sr.NO_MATE
PG_E_INVALID = -1


@pytest.fixture(scope="module")
def crafted():
    runs, ncontigs, lens_b, params, want = br.crafted_runs()
    return runs, ncontigs, lens_b, params, br.blocks(runs, lens_b, **params)


def _call(ctx, runs, ncontigs, lens_b, cap=None, **params):
    from panagram_amd import engine
    runs = np.asarray(runs, np.int64).reshape(-1, 4)
    return engine.run_blocks(ctx, runs[:, 0], runs[:, 1], runs[:, 2], runs[:, 3], ncontigs, lens_b, cap=cap, **params)


def _same_blocks(got, want, ncontigs, tag=""):
    arrs, per = got[:8], got[8]
    assert len(arrs[0]) == len(want), (tag, len(arrs[0]), len(want))
    have = np.stack(arrs, axis=1).astype(np.int64)
    bad = np.flatnonzero((have != want).any(axis=1))
    assert not len(bad), (tag, bad[:5].tolist(), have[bad[:5]].tolist(), want[bad[:5]].tolist())
    assert np.array_equal(per.astype(np.int64), np.bincount(want[:, 0], minlength=ncontigs)[:ncontigs]), tag


def test_run_blocks_on_the_crafted_list(ctx, crafted):
    runs, ncontigs, lens_b, params, want = crafted
    assert len(runs) > 3 * br.CHUNK + 77 and len(want) == 33
    a = _call(ctx, runs, ncontigs, lens_b, **params)
    _same_blocks(a, want, ncontigs)
    b = _call(ctx, runs, ncontigs, lens_b, **params)  # the same on every call
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("params", [dict(min_run=1, max_gap=5000, max_shift=10), dict(min_run=6, max_gap=5000, max_shift=10),
                                    dict(min_run=3, max_gap=4999, max_shift=10), dict(min_run=3, max_gap=5000, max_shift=9),
                                    dict(min_run=3, max_gap=5001, max_shift=10), dict(min_run=3, max_gap=6, max_shift=0),
                                    dict(min_run=1, max_gap=(1 << 31) - 1, max_shift=(1 << 31) - 1)],
                         ids=["keep-all", "drop-all", "gap-minus-one", "shift-minus-one", "gap-plus-one", "narrow", "widest"])
def test_run_blocks_on_the_crafted_list_under_other_parameters(ctx, crafted, params):
    """every run kept (the strays break the blocks), none kept, one bound moved by one at a time — the pairs of the crafted
    list that sit at a bound, or past one bound alone, change sides — links refused all over, and the widest parameters the
    call takes: 64-bit sums of 32-bit operands"""
    runs, ncontigs, lens_b, _, _ = crafted
    want = br.blocks(runs, lens_b, **params)
    assert (len(want) == 0) == (params["min_run"] == 6)
    _same_blocks(_call(ctx, runs, ncontigs, lens_b, **params), want, ncontigs, str(params))


def test_run_blocks_capacity_protocol(ctx, crafted):
    runs, ncontigs, lens_b, params, want = crafted
    total = len(want)
    per_want = np.bincount(want[:, 0], minlength=ncontigs)
    for cap in (0, total - 1):
        *arrs, per, got_total = _call(ctx, runs, ncontigs, lens_b, cap=cap, **params)
        assert got_total == total and np.array_equal(per.astype(np.int64), per_want), cap
        assert all(len(a) == cap and (a == NO).all() for a in arrs), cap  # nothing is written
    *arrs, per, got_total = _call(ctx, runs, ncontigs, lens_b, cap=total, **params)
    assert got_total == total
    _same_blocks((*arrs, per), want, ncontigs, "cap = total")
    *arrs, per, got_total = _call(ctx, runs, ncontigs, lens_b, cap=total + 5, **params)
    _same_blocks((*[a[:total] for a in arrs], per), want, ncontigs, "cap > total")
    assert all((a[total:] == NO).all() for a in arrs)


def test_run_blocks_invalid_arguments(ctx):
    from panagram_amd import engine
    good = [[0, 0, 4, 10 << 1], [0, 10, 14, 20 << 1], [1, 2, 6, (50 << 1) | 1]]
    lens_b = [60, 40]
    ok = dict(min_run=1, max_gap=100, max_shift=10)
    assert len(_call(ctx, good, 2, lens_b, **ok)[0]) == 2

    def refused(runs, ncontigs=2, lens=lens_b, **kw):
        with pytest.raises(engine.PanagramHipError) as ei:
            _call(ctx, runs, ncontigs, lens, **{**ok, **kw})
        assert ei.value.code == PG_E_INVALID, ei.value
    refused([good[1], good[0], good[2]])                           # not sorted by start
    refused([good[2], good[0], good[1]])                           # not sorted by contig
    refused([good[0], [0, 3, 8, 20 << 1], good[2]])                # overlapping
    refused([good[0], [0, 10, 10, 20 << 1], good[2]])              # end == start
    refused([good[0], [0, 10, 9, 20 << 1], good[2]])               # end < start
    refused([good[0], [0, 10, 14, NO], good[2]])                   # no mate
    refused([good[0], [0, 10, 14, 97 << 1], good[2]])              # strand +: the last k-mer at 100 = sum(lensB)
    refused([good[0], good[1], [1, 2, 6, (2 << 1) | 1]])           # strand -: the last k-mer at -1
    refused([good[0], good[1], [1, 2, 6, (100 << 1) | 1]])         # strand -: the first k-mer at sum(lensB)
    refused(good, ncontigs=1)                                      # a contig of A that does not exist
    refused(good, lens=[])                                         # no B at all
    refused(good, min_run=0)
    refused(good, max_gap=0)
    refused(good, max_gap=1 << 31)
    refused(good, max_shift=1 << 31)
    # the bounds themselves are taken: a run that ends on B's last position, on both strands
    edge = [[0, 0, 4, 96 << 1], [1, 2, 6, (3 << 1) | 1]]
    assert len(_call(ctx, edge, 2, lens_b, min_run=1, max_gap=(1 << 31) - 1, max_shift=(1 << 31) - 1)[0]) == 2
    with pytest.raises(ValueError):
        _call(ctx, good, 2, lens_b, min_run=1, max_gap=1 << 32, max_shift=0)
    # more than 2^31 - 1 runs: refused on the count alone, before an array is read
    cols = [np.ascontiguousarray(np.array(good, np.uint32)[:, i]) for i in range(4)]
    lb, per, total = np.array(lens_b, np.uint64), np.zeros(2, np.uint64), C.c_uint64()
    rc = ctx._lib.pg_run_blocks(ctx._h, *[engine._ptr(c) for c in cols], 1 << 31, 2, 2, engine._ptr(lb), 1, 100, 10, 0, *[None] * 8,
                                engine._ptr(per), C.byref(total))
    assert rc == PG_E_INVALID and "runs" in ctx._lib.pg_last_error().decode()
    # ... and a missing count or array
    assert ctx._lib.pg_run_blocks(ctx._h, *[engine._ptr(c) for c in cols], 3, 2, 2, engine._ptr(lb), 1, 100, 10, 0, *[None] * 8,
                                  engine._ptr(per), None) == PG_E_INVALID
    assert ctx._lib.pg_run_blocks(ctx._h, *[engine._ptr(c) for c in cols], 3, 2, 2, engine._ptr(lb), 1, 100, 10, 4, *[None] * 8,
                                  engine._ptr(per), C.byref(total)) == PG_E_INVALID


def test_run_blocks_empty_lists(ctx):
    got = _call(ctx, np.zeros((0, 4), np.int64), 0, [], min_run=1, max_gap=10, max_shift=1)
    assert all(len(a) == 0 for a in got)
    got = _call(ctx, np.zeros((0, 4), np.int64), 3, [100, 0], min_run=1, max_gap=10, max_shift=1)
    assert all(len(a) == 0 for a in got[:8]) and got[8].tolist() == [0, 0, 0]
    *arrs, per, total = _call(ctx, np.zeros((0, 4), np.int64), 2, [100], cap=4, min_run=1, max_gap=10, max_shift=1)
    assert total == 0 and per.tolist() == [0, 0] and all((a == NO).all() for a in arrs)


def test_with_unit_gap_the_blocks_are_the_runs_of_mate_runs(ctx):
    """random stretches of mates over three contigs, several chunks of runs: engine.mate_runs' runs, handed to run_blocks with
    min_run = 1 and max_gap = 1, come back as they went in"""
    from panagram_amd import engine
    rng = np.random.default_rng(23)
    nk = [30011, 1, 9000]
    m = np.full(sum(nk), NO, np.int64)
    at = 0
    while at < len(m):
        n = min(int(rng.integers(1, 6)), len(m) - at)
        pos, strand = int(rng.integers(10, 10 ** 6)), int(rng.integers(0, 2))
        j = np.arange(n)
        m[at:at + n] = ((pos + j) << 1) if strand == 0 else (((pos - j) << 1) | 1)
        at += n + int(rng.integers(0, 2))
    m = m.astype(np.uint32)
    rc, rs, re_, rm, per = engine.mate_runs(ctx, m, nk)
    want = sr.runs(m, nk)
    assert len(want) > 2 * br.CHUNK and np.array_equal(np.stack([rc, rs, re_, rm], axis=1).astype(np.int64), want)
    got = engine.run_blocks(ctx, rc, rs, re_, rm, len(nk), [10 ** 6 + 10], min_run=1, max_gap=1, max_shift=0)
    n = want[:, 2] - want[:, 1]
    last = np.where(want[:, 3] & 1, want[:, 3] - 2 * (n - 1), want[:, 3] + 2 * (n - 1))
    ident = np.column_stack([want, last, n, np.ones_like(n), np.zeros_like(n)])
    _same_blocks(got, ident, len(nk))
    assert np.array_equal(got[8], per)
