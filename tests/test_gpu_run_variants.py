"""GPU: k_link_variants (panagram_amd/csrc/pg_variants.hip) through pg_run_variants on the crafted run list of
tests/variants_ref.py — no hashing involved, the kernel compares whatever bases lie at the coordinates — against the numpy model,
exactly, order and every field.  Then other parameters, the capacity protocol, every invalid argument and the empty list."""
import ctypes as C

import numpy as np
import pytest

from tests import variants_ref as vr

pytestmark = pytest.mark.gpu

NO32, NO64 = 0xFFFFFFFF, (1 << 64) - 1
PG_E_INVALID = -1


@pytest.fixture(scope="module")
def crafted():
    runs, a, b, k, params, marks = vr.crafted()
    return runs, a, b, k, params, vr.variants(runs, a, b, k, **params)


@pytest.fixture(scope="module")
def sides(ctx, crafted):
    from panagram_amd import engine
    _, a, b, _, _, _ = crafted
    ssa, ssb = engine.SeqSet.from_host(ctx, a), engine.SeqSet.from_host(ctx, b)
    yield ssa, ssb
    ssa.close()
    ssb.close()


def _call(ctx, sides, k, runs, cap=None, **params):
    from panagram_amd import engine
    runs = np.asarray(runs, np.int64).reshape(-1, 4)
    return engine.run_variants(ctx, k, sides[0], sides[1], runs[:, 0], runs[:, 1], runs[:, 2], runs[:, 3], cap=cap, **params)


def _same_records(got, model, tag=""):
    arrs, cls, links = got[:9], got[9], got[10]
    want = model["records"]
    print(tag, "records", len(arrs[0]), "of", len(want), "classes", cls.tolist(), model["classes"], "links", links, model["links"])
    assert cls.astype(np.int64).tolist() == model["classes"] and links == model["links"] == int(cls.sum()), tag
    assert len(arrs[0]) == len(want), (tag, len(arrs[0]), len(want))
    have = np.stack(arrs[:7], axis=1).astype(np.int64)
    bad = np.flatnonzero((have != want).any(axis=1))
    assert not len(bad), (tag, bad[:5].tolist(), have[bad[:5]].tolist(), want[bad[:5]].tolist())
    words = np.stack(arrs[7:], axis=1)
    bad = np.flatnonzero((words != model["words"]).any(axis=1))
    assert not len(bad), (tag, bad[:5].tolist(), words[bad[:5]].tolist(), model["words"][bad[:5]].tolist(), want[bad[:5]].tolist())


def test_run_variants_on_the_crafted_list(ctx, crafted, sides):
    runs, _, _, k, params, model = crafted
    assert len(runs) > 3 * vr.CHUNK + 77 and all(n > 0 for n in model["classes"])
    a = _call(ctx, sides, k, runs, **params)
    _same_records(a, model)
    b = _call(ctx, sides, k, runs, **params)  # the same on every call
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("params", [dict(min_run=1, max_gap=5000, max_shift=60), dict(min_run=6, max_gap=5000, max_shift=60),
                                    dict(min_run=3, max_gap=4999, max_shift=60), dict(min_run=3, max_gap=5000, max_shift=59),
                                    dict(min_run=3, max_gap=5001, max_shift=60), dict(min_run=3, max_gap=5000, max_shift=61),
                                    dict(min_run=3, max_gap=vr.MAX_GAP, max_shift=(1 << 31) - 1)],
                         ids=["keep-all", "drop-all", "gap-minus-one", "shift-minus-one", "gap-plus-one", "shift-plus-one", "widest"])
def test_run_variants_on_the_crafted_list_under_other_parameters(ctx, crafted, sides, params):
    """every run kept (the strays break the blocks), none kept, one bound moved by one at a time — the pairs of the crafted list
    that sit at a bound, or past one bound alone, change sides — and the widest parameters the call takes"""
    runs, a, b, k, _, base = crafted
    model = vr.variants(runs, a, b, k, **params)
    assert (model["links"] == 0) == (params["min_run"] == 6)
    if params["min_run"] == 3:
        assert model["links"] != base["links"] or params["max_gap"] == vr.MAX_GAP, params
    _same_records(_call(ctx, sides, k, runs, **params), model, str(params))


def test_run_variants_capacity_protocol(ctx, crafted, sides):
    runs, _, _, k, params, model = crafted
    total = len(model["records"])
    for cap in (0, total - 1):
        *arrs, cls, links, got_total = _call(ctx, sides, k, runs, cap=cap, **params)
        assert got_total == total and links == model["links"] and cls.astype(np.int64).tolist() == model["classes"], cap
        assert all(len(x) == cap for x in arrs) and all((x == NO32).all() for x in arrs[:7]) and all((x == NO64).all() for x in arrs[7:]), cap
    *arrs, cls, links, got_total = _call(ctx, sides, k, runs, cap=total, **params)
    assert got_total == total
    _same_records((*arrs, cls, links), model, "cap = total")
    *arrs, cls, links, got_total = _call(ctx, sides, k, runs, cap=total + 5, **params)
    _same_records((*[x[:total] for x in arrs], cls, links), model, "cap > total")
    assert all((x[total:] == NO32).all() for x in arrs[:7]) and all((x[total:] == NO64).all() for x in arrs[7:])


def test_run_variants_invalid_arguments(ctx):
    from panagram_amd import engine
    k = 5
    ssa = engine.SeqSet.from_host(ctx, [b"ACGTACGGTTCAGGCATTAGCCATG" * 2, b"TTGACCAGTACCGATAGGCA" * 2])   # 50 and 40 bases
    ssb = engine.SeqSet.from_host(ctx, [b"GGATCCATTGACGTTAGCAATCGGATACCA" * 2, b"CATGGTACCAGTTAGACCAT" * 2])  # 60 and 40
    try:
        good = [[0, 0, 4, 10 << 1], [0, 10, 14, 20 << 1], [1, 2, 6, (50 << 1) | 1]]
        ok = dict(min_run=1, max_gap=100, max_shift=10)
        got = _call(ctx, (ssa, ssb), k, good, **ok)
        assert got[10] == 1 and int(got[9].sum()) == 1

        def refused(runs, k=k, a=ssa, b=ssb, **kw):
            with pytest.raises(engine.PanagramHipError) as ei:
                _call(ctx, (a, b), k, runs, **{**ok, **kw})
            assert ei.value.code == PG_E_INVALID, ei.value
        refused([good[1], good[0], good[2]])                           # not sorted by start
        refused([good[2], good[0], good[1]])                           # not sorted by contig
        refused([good[0], [0, 3, 8, 20 << 1], good[2]])                # overlapping
        refused([good[0], [0, 10, 10, 20 << 1], good[2]])              # end == start
        refused([good[0], [0, 10, 14, NO32], good[2]])                 # no mate
        refused([good[0], [0, 10, 14, 97 << 1], good[2]])              # strand +: the last k-mer at 100 = B's bases
        refused([good[0], good[1], [1, 2, 6, (2 << 1) | 1]])           # strand -: the last k-mer at -1
        refused([good[0], good[1], [2, 2, 6, (50 << 1) | 1]])          # a contig of A that does not exist
        refused([good[0], [0, 43, 47, 20 << 1], good[2]])              # the last k-mer's bases leave the contig of A: 47 + 4 > 50
        refused([good[0], [0, 10, 14, 53 << 1], good[2]])              # ... leave the contig of B: 53 + 4 + 4 > 60
        refused([good[0], good[1], [1, 2, 6, (62 << 1) | 1]])          # ... on strand -: [59, 67) straddles B's contig edge at 60
        refused(good, min_run=0)
        refused(good, max_gap=0)
        refused(good, max_gap=vr.MAX_GAP + 1)
        refused(good, max_shift=1 << 31)
        refused(good, k=0)
        refused(good, k=33)
        # the bounds themselves are taken: runs that end on the last base of their contigs, on both strands
        edge = [[0, 42, 46, 52 << 1], [1, 32, 36, (63 << 1) | 1]]
        got = _call(ctx, (ssa, ssb), k, edge, min_run=1, max_gap=vr.MAX_GAP, max_shift=(1 << 31) - 1)
        assert got[10] == 0 and len(got[0]) == 0
        with pytest.raises(ValueError):
            _call(ctx, (ssa, ssb), k, good, min_run=1, max_gap=1 << 32, max_shift=0)
        # a missing count or array
        cols = [np.ascontiguousarray(np.array(good, np.uint32)[:, i]) for i in range(4)]
        cls, links, total = np.zeros(6, np.uint64), C.c_uint64(), C.c_uint64()
        head = (ctx._h, k, ssa._h, ssb._h, *[engine._ptr(c) for c in cols], 3, 1, 100, 10)
        assert ctx._lib.pg_run_variants(*head, 0, *[None] * 9, engine._ptr(cls), C.byref(links), None) == PG_E_INVALID
        assert ctx._lib.pg_run_variants(*head, 0, *[None] * 9, None, C.byref(links), C.byref(total)) == PG_E_INVALID
        assert ctx._lib.pg_run_variants(*head, 4, *[None] * 9, engine._ptr(cls), C.byref(links), C.byref(total)) == PG_E_INVALID
        assert ctx._lib.pg_run_variants(*head, 0, *[None] * 9, engine._ptr(cls), C.byref(links), C.byref(total)) == 0 and links.value == 1
    finally:
        ssa.close()
        ssb.close()


def test_run_variants_empty_lists(ctx):
    from panagram_amd import engine
    ssa, ssb = engine.SeqSet.from_host(ctx, [b"ACGTTGCA" * 4, b"ACCA"]), engine.SeqSet.from_host(ctx, [b"TTGACCAG" * 4])
    try:
        got = _call(ctx, (ssa, ssb), 5, np.zeros((0, 4), np.int64), min_run=1, max_gap=10, max_shift=1)
        assert all(len(x) == 0 for x in got[:9]) and got[9].tolist() == [0] * 6 and got[10] == 0
        *arrs, cls, links, total = _call(ctx, (ssa, ssb), 5, np.zeros((0, 4), np.int64), cap=4, min_run=1, max_gap=10, max_shift=1)
        assert total == 0 and links == 0 and all((x == NO32).all() for x in arrs[:7])
        # one run: kept, no link
        got = _call(ctx, (ssa, ssb), 5, [[0, 0, 4, 3 << 1]], min_run=1, max_gap=10, max_shift=1)
        assert all(len(x) == 0 for x in got[:9]) and got[10] == 0
    finally:
        ssa.close()
        ssb.close()
