"""GPU: k_pattern_counts (panagram_amd/csrc/pg_patterns.hip) on rows PLANTED into a rows container (tests/rows_craft.py), every
byte that is not a row byte holding 0xFF.  Keys and counts are exactly equal to the numpy restatement (tests/patterns_ref.py,
tied on the CPU to DataFrame.value_counts(): tests/test_patterns_cpu.py), and the counts add up to the windows' sampled rows.

Which path runs for which case: all genomes of N <= 64 selected — the key is the row's bytes (k_pattern_counts<true>); any
other selection — fields moved under the selection words (k_pattern_counts<false>).  A wave takes 64 sampled rows, a tile 256, a
workgroup's chunk engine.PATTERN_CHUNK; a workgroup's LDS table has 1024 slots, beyond them heads go to the global table."""
import ctypes as C

import numpy as np
import pytest

from tests import rows_craft as rc
from tests.patterns_ref import ref_keys
from tests.test_gpu_find import windows

pytestmark = pytest.mark.gpu

K = 21
ALL_N = [1, 7, 8, 9, 31, 32, 33, 63, 64]
STRIDES = [1, 3, 100]
PG_E_INVALID = -1
CANARY = 0xDEADBEEFDEADBEEF


def _chunk():
    from panagram_amd import engine
    return engine.PATTERN_CHUNK


def _nks():
    return [3 * _chunk() + 77, 1111]


def _raw(res, contigs, starts, ends, sel, cap, keys, counts, stride=1):
    contigs, starts, ends = np.asarray(contigs, np.uint32), np.asarray(starts, np.uint64), np.asarray(ends, np.uint64)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    nd, rows, exceeded = C.c_uint64(12345), C.c_uint64(12345), C.c_int(7)
    code = res._lib.pg_result_pattern_counts(res._h, 1, stride, len(contigs), vp(contigs), vp(starts), vp(ends), vp(sel), cap,
                                             vp(keys), vp(counts), C.byref(nd), C.byref(rows), C.byref(exceeded))
    return code, nd.value, rows.value, exceeded.value


def _want(rows, n, contigs, starts, ends, stride, select):
    """tests/patterns_ref.py's ref_pattern_counts, the keys of a contig (ref_keys) computed once for all of its windows"""
    keys = [ref_keys(r, n, stride, select) for r in rows]
    k, c = np.unique(np.concatenate([keys[int(ci)][int(s):int(e)] for ci, s, e in zip(contigs, starts, ends)]), return_counts=True)
    return k.astype(np.uint64), c.astype(np.uint64)


def _check(res, rows, n, stride, select, tag, all_genomes=False, words=None):
    """equality with the model and conservation; select: the columns, all_genomes: passed as no selection at all"""
    from panagram_amd import engine
    contigs, starts, ends = windows([len(r) for r in rows], stride)
    sel = None if all_genomes else (rc.words_of(n, select) if words is None else words)
    exceeded, total, keys, counts = res._patterns(contigs, starts, ends, sel, 1, stride, engine.PATTERN_FIRST_CAP)
    want_k, want_c = _want(rows, n, contigs, starts, ends, stride, select)
    assert not exceeded, (tag, n, stride)
    assert keys.dtype == np.uint64 and counts.dtype == np.uint64
    assert np.array_equal(keys, want_k), (tag, n, stride, len(keys), len(want_k))
    assert np.array_equal(counts, want_c), (tag, n, stride)
    assert int(counts.sum()) == total == int((ends - starts).sum()), (tag, n, stride)
    return keys, counts


@pytest.fixture
def planted(ctx, request):
    n = request.param
    res = rc.container(ctx, K, n, _nks(), colsums=False)
    try:
        rc.plant(res, [rc.zeros(nk, n) for nk in _nks()], poison=0xFF)
        res.rows_epilogue()  # (a rows container is read once its statistics have been enqueued)
        yield res, n
    finally:
        res.close()


def _plant(res, rows):
    rc.plant(res, rows, poison=0xFF)
    return rows


@pytest.mark.parametrize("planted", ALL_N, indirect=True)
def test_all_genomes_selected(planted):
    res, n = planted
    nks = _nks()
    every = list(range(n))
    top = (1 << n) - 1
    for stride in STRIDES:
        rows = _plant(res, [rc.ones(nk, n) for nk in nks])  # (N = 64: the all-ones key, the table's empty word)
        keys, _ = _check(res, rows, n, stride, every, "ones", all_genomes=True)
        assert keys.tolist() == [top]
        rows = _plant(res, [rc.zeros(nk, n) for nk in nks])
        keys, _ = _check(res, rows, n, stride, every, "zeros", all_genomes=True)
        assert keys.tolist() == [0]
        rows = _plant(res, [rc.ramp(nk, n) for nk in nks])
        keys, _ = _check(res, rows, n, stride, every, "ramp", all_genomes=True)
        assert stride != 1 or (len(keys) == n + 1 and keys[-1] == top)
        rows = _plant(res, [rc.checker(nk, n) for nk in nks])  # (no run longer than 1 at an odd stride)
        keys, _ = _check(res, rows, n, stride, every, "checker", all_genomes=True)
        assert len(keys) == (1 if stride % 2 == 0 else 2)
        for length in (63, 64):  # runs that end on and beside a wave's edge
            rows = _plant(res, [rc.bursts(nk, n, length) for nk in nks])
            keys, _ = _check(res, rows, n, stride, every, f"bursts {length}", all_genomes=True)
            assert stride != 1 or keys.tolist() == [0, top]
        if n % 8:
            clean = [rc.dense(nk, n, 40 + n + i) for i, nk in enumerate(nks)]
            _plant(res, [rc.with_pad_bits(r, n) for r in clean])
            _check(res, clean, n, stride, every, "pad bits", all_genomes=True)
            # ... and the same with the selection spelt out, every bit of its words set
            _check(res, clean, n, stride, every, "pad bits, full words", words=np.full((n + 31) // 32, 0xFFFFFFFF, np.uint32))
    # ones beside other rows (N = 64: the all-ones key appended behind the table's keys)
    rows = _plant(res, [rc.back_to_back(nk, [(1, lambda m: rc.ones(m, n)), (1, lambda m: rc.dense(m, n, 7)), (1, lambda m: rc.ones(m, n))])
                        for nk in nks])
    keys, counts = _check(res, rows, n, 1, every, "ones and dense", all_genomes=True)
    assert keys[-1] == top and counts[-1] >= 2 * (nks[0] // 3)
    # determinism: two calls, identical arrays
    contigs, starts, ends = windows(nks, 1)
    a = res.pattern_counts(contigs, starts, ends)
    b = res.pattern_counts(contigs, starts, ends)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[0], keys)
    # no window, and empty windows only: zero patterns
    for c, s, e in [([], [], []), ([0, 1], [5, 0], [5, 0])]:
        k, cnt = res.pattern_counts(c, s, e)
        assert k.shape == (0,) and cnt.shape == (0,) and k.dtype == np.uint64
        code, nd, total, exceeded = _raw(res, c, s, e, None, 0, None, None)
        assert (code, nd, total, exceeded) == (0, 0, 0, 0)


@pytest.mark.parametrize("planted", [8, 16], indirect=True)
def test_dense_rows(planted):
    """N = 8: all 256 patterns; N = 16: some 7 000 distinct keys per chunk of 8192 rows, far more than a workgroup's LDS table
    holds — most heads go straight to the global table"""
    res, n = planted
    rows = _plant(res, [rc.dense(nk, n, 60 + n + i) for i, nk in enumerate(_nks())])
    for stride in STRIDES:
        keys, _ = _check(res, rows, n, stride, list(range(n)), "dense", all_genomes=True)
        if stride == 1:
            assert len(keys) == 256 if n == 8 else len(keys) > 4 * 1024


def _straddling(n):
    """64 columns of N = 130 around every word boundary: 16 around each of 32, 64 and 96, the last 10, and 6 low ones"""
    cols = [0, 2, 4, 6, 8, 10] + list(range(24, 40)) + list(range(56, 72)) + list(range(88, 104)) + list(range(120, 130))
    assert len(cols) == 64 and n == 130
    return cols


# (the last two: rows of whole words, 8 and 32 bytes, off the low columns, with a field that crosses a word boundary)
SELECTIONS = [(9, [0, 8]), (33, [31, 32]), (130, None), (1000, [0, 511, 999]), (64, list(range(63))), (64, [0, 63]),
              (256, [31, 32, 255])]


def _selection_ids():
    """N<n>, and N<n>-<columns> for a second selection at the same N"""
    seen = set()
    for n, s in SELECTIONS:
        yield f"N{n}" if n not in seen else f"N{n}-" + "_".join(map(str, s))
        seen.add(n)


@pytest.mark.parametrize("planted,select", [pytest.param(n, s, id=i) for (n, s), i in zip(SELECTIONS, _selection_ids())],
                         indirect=["planted"])
def test_selections(planted, select):
    """(N = 64, the 63 columns below the top one: the fast path's condition is false by one bit)"""
    res, n = planted
    select = _straddling(n) if select is None else select
    nks = _nks()
    clean = [rc.dense(nk, n, 90 + n + i) for i, nk in enumerate(nks)]
    for stride in STRIDES:
        rows = _plant(res, clean)
        _check(res, rows, n, stride, select, "dense")
        rows = _plant(res, [rc.ramp(nk, n) for nk in nks])
        _check(res, rows, n, stride, select, "ramp")
        rows = _plant(res, [rc.ones(nk, n) for nk in nks])
        keys, _ = _check(res, rows, n, stride, select, "ones")
        assert keys.tolist() == [(1 << len(select)) - 1]
        rows = _plant(res, [rc.bursts(nk, n, 64) for nk in nks])
        _check(res, rows, n, stride, select, "bursts 64")
    if n % 8:
        _plant(res, [rc.with_pad_bits(r, n) for r in clean])
        _check(res, clean, n, 1, select, "pad bits")
    contigs, starts, ends = windows(nks, 1)
    a = res.pattern_counts(contigs, starts, ends, rc.words_of(n, select))
    b = res.pattern_counts(contigs, starts, ends, rc.words_of(n, select))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and len(a[0]) > 0


def test_capacity(ctx, monkeypatch):
    """dense rows at N = 64, every row distinct: the table of a call is max(1024, the power of two >= 2 * cap) slots"""
    from panagram_amd import engine
    n, ch = 64, _chunk()
    nks = [ch + 700, 50]
    rows = [rc.dense(nk, n, 5 + i) for i, nk in enumerate(nks)]
    key0 = ref_keys(rows[0], n, 1, range(n))
    assert len(np.unique(key0)) == nks[0]  # every row of contig 0 is distinct
    res = rc.container(ctx, K, n, nks, colsums=False)
    try:
        rc.plant(res, rows, poison=0xFF)
        res.rows_epilogue()
        big = ([0], [100], [100 + ch + 5])
        assert ch + 5 > 2048  # more distinct keys than the slots cap = 1000 allocates
        keys, counts = np.full(1000, CANARY, np.uint64), np.full(1000, CANARY, np.uint64)
        code, _, total, exceeded = _raw(res, *big, None, 1000, keys, counts)
        assert (code, total, exceeded) == (0, ch + 5, 1)
        assert (keys == CANARY).all() and (counts == CANARY).all()
        code, _, total, exceeded = _raw(res, *big, None, 0, None, None)  # cap = 0 takes NULL arrays
        assert (code, total, exceeded) == (0, ch + 5, 1)
        # exactly D distinct keys: cap = D passes, cap = D - 1 does not
        D = 300
        want = np.sort(key0[7:7 + D])
        keys, counts = np.full(D, CANARY, np.uint64), np.full(D, CANARY, np.uint64)
        code, nd, total, exceeded = _raw(res, [0], [7], [7 + D], None, D, keys, counts)
        assert (code, nd, total, exceeded) == (0, D, D, 0)
        assert np.array_equal(keys, want) and (counts == 1).all()
        keys, counts = np.full(D, CANARY, np.uint64), np.full(D, CANARY, np.uint64)
        code, _, total, exceeded = _raw(res, [0], [7], [7 + D], None, D - 1, keys, counts)
        assert (code, total, exceeded) == (0, D, 1) and (keys == CANARY).all() and (counts == CANARY).all()
        # the wrapper's retry: 256, then 4096, then 65536 patterns of room
        monkeypatch.setattr(engine, "PATTERN_FIRST_CAP", 256)
        k, c = res.pattern_counts(*big)
        assert np.array_equal(k, np.sort(key0[100:100 + ch + 5])) and (c == 1).all()
        monkeypatch.setattr(engine, "PATTERN_MAX_CAP", 4096)
        with pytest.raises(ValueError, match="4096.*fewer genomes"):
            res.pattern_counts(*big)
    finally:
        res.close()
    # rows of ones at N = 64: one pattern, which the table never holds
    res = rc.container(ctx, K, n, [500], colsums=False)
    try:
        rc.plant(res, [rc.ones(500, n)], poison=0xFF)
        res.rows_epilogue()
        keys, counts = np.full(1, CANARY, np.uint64), np.full(1, CANARY, np.uint64)
        code, nd, total, exceeded = _raw(res, [0], [0], [500], None, 1, keys, counts)
        assert (code, nd, total, exceeded) == (0, 1, 500, 0) and keys.tolist() == [2 ** 64 - 1] and counts.tolist() == [500]
        code, _, total, exceeded = _raw(res, [0], [0], [500], None, 0, None, None)
        assert (code, total, exceeded) == (0, 500, 1)
    finally:
        res.close()


def test_refused_calls(ctx):
    """each is PG_E_INVALID before anything is launched"""
    from panagram_amd._lib import PanagramHipError
    for n, sel, msg in [(130, rc.words_of(130, range(3, 68)), "65 genomes selected"), (65, None, "65 genomes selected"),
                        (12, np.zeros(1, np.uint32), "no genome selected"),
                        (12, np.array([0xFFFFF000], np.uint32), "no genome selected")]:  # (bits at and past N only)
        res = rc.container(ctx, K, n, [300, 50], colsums=False)
        try:
            rc.plant(res, [rc.dense(300, n, 2), rc.dense(50, n, 3)], poison=0xFF)
            res.rows_epilogue()
            keys, counts = np.full(8, CANARY, np.uint64), np.full(8, CANARY, np.uint64)
            code, _, _, _ = _raw(res, [0], [0], [300], sel, 8, keys, counts)
            assert code == PG_E_INVALID and (keys == CANARY).all() and (counts == CANARY).all()
            with pytest.raises(PanagramHipError, match=msg) as ei:
                res.pattern_counts([0], [0], [300], sel)
            assert ei.value.code == PG_E_INVALID
            if n == 12:  # a window past its contig, and its neighbours in test_gpu_find.py's list
                ok = rc.words_of(n, [1, 5])
                for contigs, starts, ends, stride, msg in [
                        ([1], [0], [51], 1, "window 0: sampled row 50 (x 1) past the 50 rows of contig 1"),
                        ([0], [0], [101], 3, "window 0: sampled row 100 (x 3) past the 300 rows of contig 0"),
                        ([2], [0], [1], 1, "window 0: contig 2 out of range"),
                        ([0], [9], [8], 1, "window 0: start 9 past end 8"),
                        ([0], [0], [10], 0, "pg_result_pattern_counts: stride must be >= 1")]:
                    with pytest.raises(PanagramHipError) as ei:
                        res.pattern_counts(contigs, starts, ends, ok, stride=stride)
                    assert ei.value.code == PG_E_INVALID and str(ei.value).endswith(msg), (str(ei.value), msg)
                # the last sampled rows that do fit
                k, c = res.pattern_counts([0, 1], [0, 0], [100, 17], ok, stride=3)
                assert int(c.sum()) == 117 and len(k) <= 4
        finally:
            res.close()
