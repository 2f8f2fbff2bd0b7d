"""GPU: k_find_runs (panagram_amd/csrc/pg_find.hip) on rows PLANTED into a rows container (tests/rows_craft.py), every byte
that is not a row byte holding 0xFF.  Every result is exactly equal — order included — to the numpy restatement
(tests/find_ref.py, tied on the CPU to scripts/query_index.py's expression: tests/test_find_cpu.py).

Which kernel runs for which N: N <= 128 k_find_runs<4, .> (the masks in registers), beyond k_find_runs<0, .> (the masks in
LDS).  A wave takes 64 sampled rows, a tile is 256, a workgroup's chunk engine.FIND_CHUNK; chunks count from their window's
first sampled row."""
import ctypes as C

import numpy as np
import pytest

from tests import rows_craft as rc
from tests.find_ref import ref_match
from tests.test_gpu_pair_counts import windows as pair_windows

pytestmark = pytest.mark.gpu

K = 21
FIND_N = [1, 2, 7, 8, 9, 31, 32, 33, 64, 65, 127, 128, 129, 130, 256, 1000]
STRIDES = [1, 3, 100]
PG_E_INVALID = -1


def _chunk():
    from panagram_amd import engine
    return engine.FIND_CHUNK


def _nks():
    return [3 * _chunk() + 77, 1111]


def windows(nks, stride):
    """tests/test_gpu_pair_counts.py's window set — an empty window, lengths around 64 and 256 from starts that are no
    multiples of 64, windows ending on each contig's last row, both contigs whole — and: windows INSIDE contig 0 whose row
    before s and row at e exist (both match when the rows are ones: the run must be cut to [s, e)), of a chunk and a bit, of
    exactly one and two chunks; contig 1 from its row 0, right behind the poisoned padding"""
    c, s, e = pair_windows(nks, stride)
    ns = [(nk - 1) // stride + 1 for nk in nks]
    ch = _chunk()
    extra = [(1, 0, min(64, ns[1])), (1, 0, 1)]
    for a, b in [(1, ns[0] - 1), (100, 100 + ch + 5), (3, 3 + ch), (64, 64 + 2 * ch), (ch - 1, ch + 1), (ch, 2 * ch + 1),
                 (255, 257), (5, ns[0] - 5)]:
        if a < b < ns[0]:
            extra.append((0, a, b))
    ec, es, ee = (np.array(x) for x in zip(*extra))
    return (np.concatenate([c, ec.astype(np.uint32)]), np.concatenate([s, es.astype(np.uint64)]),
            np.concatenate([e, ee.astype(np.uint64)]))


def _runs_of(m, s, e):
    d = np.diff(np.concatenate([[0], m[s:e].astype(np.int8), [0]]))
    return np.flatnonzero(d == 1) + s, np.flatnonzero(d == -1) + s, int(m[s:e].sum())


def _want(rows, n, contigs, starts, ends, stride, have, lack, min_have, max_lack):
    """(runs [total, 3], matched [nwin]) by tests/find_ref.py: ref_find_runs window by window, the match vector of a contig
    (ref_match, which ref_find_runs slices) computed once for all of its windows"""
    m = [ref_match(r, n, stride, have, lack, min_have, max_lack) for r in rows]
    out, matched = [], []
    for i, (c, s, e) in enumerate(zip(contigs, starts, ends)):
        rs, re, k = _runs_of(m[int(c)], int(s), int(e))
        out.append(np.stack([np.full(len(rs), i, np.int64), rs, re], axis=1))
        matched.append(k)
    return np.concatenate(out), np.array(matched, np.int64)


def _check(res, rows, n, stride, have, lack, min_have, max_lack, tag, words=None):
    nks = [len(r) for r in rows]
    contigs, starts, ends = windows(nks, stride)
    hw, lw = words if words is not None else (rc.words_of(n, have), rc.words_of(n, lack))
    runs, matched = res.find_runs(contigs, starts, ends, hw, lw, min_have, max_lack, step=1, stride=stride)
    want_runs, want_matched = _want(rows, n, contigs, starts, ends, stride, have, lack, min_have, max_lack)
    assert runs.dtype == np.int64 and runs.shape == want_runs.shape, (tag, n, stride, runs.shape, want_runs.shape)
    assert np.array_equal(runs, want_runs), (tag, n, stride)
    assert np.array_equal(matched.astype(np.int64), want_matched), (tag, n, stride)
    return runs, matched, (contigs, starts, ends)


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


@pytest.mark.parametrize("planted", FIND_N, indirect=True)
def test_ones_zeros_checker_and_dense(planted):
    res, n = planted
    nks = _nks()
    every = list(range(n))
    last = [n - 1] if n > 1 else []
    # ones: one run per non-empty window, cut to it; zeros: none
    rows = _plant(res, [rc.ones(nk, n) for nk in nks])
    for stride in STRIDES:
        runs, matched, (c, s, e) = _check(res, rows, n, stride, every, [], n, 0, "ones")
        nonempty = np.flatnonzero(e > s)
        assert np.array_equal(runs[:, 0], nonempty) and np.array_equal(runs[:, 1], s[nonempty].astype(np.int64))
        assert np.array_equal(runs[:, 2], e[nonempty].astype(np.int64)) and np.array_equal(matched, e - s)
        if n > 1:
            runs, matched, _ = _check(res, rows, n, stride, [0], [n - 1], 1, 0, "ones, one lacking")
            assert len(runs) == 0 and not matched.any()
    rows = _plant(res, [rc.zeros(nk, n) for nk in nks])
    for stride in STRIDES:
        runs, matched, _ = _check(res, rows, n, stride, [0], [], 1, 0, "zeros")
        assert len(runs) == 0 and not matched.any()
        runs, matched, (c, s, e) = _check(res, rows, n, stride, [], every, 0, 0, "zeros, all lacking")
        assert len(runs) == (e > s).sum()
    # checker, rule on column 0: every other row starts a run
    rows = _plant(res, [rc.checker(nk, n) for nk in nks])
    runs, matched, (c, s, e) = _check(res, rows, n, 1, [0], [], 1, 0, "checker")
    assert (runs[:, 2] - runs[:, 1] == 1).all() and len(runs) == matched.sum() and matched[1] == nks[0] // 2
    _check(res, rows, n, 3, [0], [], 1, 0, "checker")
    _check(res, rows, n, 100, [0], [], 1, 0, "checker")  # (an even stride: column 0 is never set)
    # dense: the reference's exact rule on the first and the last column, then quorum rules
    rows = _plant(res, [rc.dense(nk, n, 60 + n + i) for i, nk in enumerate(nks)])
    half = every[: max(1, n // 2)]
    rest = every[len(half):]
    for stride in STRIDES:
        _check(res, rows, n, stride, [0], last, 1, 0, "dense exact")
        _check(res, rows, n, stride, half, rest, max(1, len(half) // 2), len(rest) // 2, "dense quorum")
        _check(res, rows, n, stride, last, [0] if n > 1 else [], len(last), 0, "dense, last column")
    # determinism: the same call twice
    contigs, starts, ends = windows(nks, 1)
    a = res.find_runs(contigs, starts, ends, rc.words_of(n, half), rc.words_of(n, rest), 1, len(rest) // 2)
    b = res.find_runs(contigs, starts, ends, rc.words_of(n, half), rc.words_of(n, rest), 1, len(rest) // 2)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and len(a[0]) > 0
    # no window, and windows without a run: empty arrays
    runs, matched = res.find_runs([], [], [], rc.words_of(n, [0]), None, 1, 0)
    assert runs.shape == (0, 3) and runs.dtype == np.int64 and matched.shape == (0,)
    runs, matched = res.find_runs(contigs, starts, ends, rc.words_of(n, [0]), None, 2, 0)  # (min_have > |H|)
    assert runs.shape == (0, 3) and matched.shape == (len(contigs),) and not matched.any()


def _burst_lengths():
    ch = _chunk()
    return [63, 64, 65, 255, 256, ch - 1, ch, ch + 1]


@pytest.mark.parametrize("planted", FIND_N, indirect=True)
def test_bursts_on_every_wave_tile_and_chunk_boundary(planted):
    """`length` matching rows, one that does not match, and again: with the windows' starts, run edges fall on, before and
    behind every wave, tile and chunk boundary"""
    res, n = planted
    for length in _burst_lengths():
        rows = _plant(res, [rc.bursts(nk, n, length) for nk in _nks()])
        for stride in STRIDES:
            runs, _, _ = _check(res, rows, n, stride, list(range(n)), [], n, 0, f"bursts {length}")
            if stride == 1:
                assert (runs[:, 2] - runs[:, 1]).max() == length


@pytest.mark.parametrize("planted", FIND_N, indirect=True)
def test_ramp_holds_the_thresholds(planted):
    """row i holds its lowest i mod (N + 1) bits: min_have and max_lack of 0, 1, N // 2 and N over every genome"""
    res, n = planted
    rows = _plant(res, [rc.ramp(nk, n) for nk in _nks()])
    every = list(range(n))
    for t in sorted({0, 1, n // 2, n}):
        for stride in (1, 3):
            runs, matched, (c, s, e) = _check(res, rows, n, stride, every, [], t, 0, f"ramp min_have {t}")
            if t == 0:
                assert np.array_equal(matched, e - s)  # min_have = 0 and no L: every row
            _check(res, rows, n, stride, [], every, 0, t, f"ramp max_lack {t}")
        _check(res, rows, n, 1, every, every, t, t, f"ramp both {t}")  # (popcount == t exactly)
    _check(res, rows, n, 1, every, [], n + 1, 0, "ramp min_have N + 1")


@pytest.mark.parametrize("planted", FIND_N, indirect=True)
def test_pad_bits_count_on_neither_side(planted):
    """rows with the bits past N in their last byte set, and mask words with every bit set (the bits at and past N too): the
    result is that of the clean rows and masks"""
    res, n = planted
    clean = [rc.dense(nk, n, 80 + n + i) for i, nk in enumerate(_nks())]
    _plant(res, [rc.with_pad_bits(r, n) for r in clean])
    every = list(range(n))
    full = np.full((n + 31) // 32, 0xFFFFFFFF, np.uint32)
    none = np.zeros((n + 31) // 32, np.uint32)
    for stride in (1, 3):
        _check(res, clean, n, stride, [], every, 0, n // 2, "pad bits, L = every genome", words=(none, full))
        _check(res, clean, n, stride, every, [], n // 2 + 1, 0, "pad bits, H = every genome", words=(full, none))
    _check(res, clean, n, 1, every, [], n, 0, "pad bits, all of H", words=(full, none))
    _check(res, clean, n, 1, [], every, 0, 0, "pad bits, none of L", words=(none, full))


def _raw(res, contigs, starts, ends, hw, lw, min_have, max_lack, cap, rs, re, stride=1):
    contigs, starts, ends = np.asarray(contigs, np.uint32), np.asarray(starts, np.uint64), np.asarray(ends, np.uint64)
    nruns, matched, total = np.zeros(len(contigs), np.uint64), np.zeros(len(contigs), np.uint64), C.c_uint64(12345)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc_ = res._lib.pg_result_find_runs(res._h, 1, stride, len(contigs), vp(contigs), vp(starts), vp(ends), vp(hw), vp(lw), min_have,
                                       max_lack, cap, vp(rs), vp(re), vp(nruns), vp(matched), C.byref(total))
    return rc_, total.value, nruns, matched


@pytest.mark.parametrize("n", [8, 130])
def test_capacity(ctx, n):
    """more runs than engine.FIND_FIRST_CAP: find_runs makes its second call; at the ABI, cap = total - 1 leaves the run arrays
    untouched and still fills the counts, cap = total fills them, cap = 0 takes NULL arrays"""
    from panagram_amd import engine
    nks = [2 * engine.FIND_FIRST_CAP + 2 * engine.FIND_CHUNK + 10, 500]
    rows = [rc.checker(nk, n) for nk in nks]
    res = rc.container(ctx, K, n, nks, colsums=False)
    try:
        rc.plant(res, rows, poison=0xFF)
        res.rows_epilogue()
        contigs, starts, ends = [0, 1, 0], [0, 0, 1001], [nks[0], nks[1], 3003]
        hw = rc.words_of(n, [0])
        runs, matched = res.find_runs(contigs, starts, ends, hw, None, 1, 0)
        want_runs, want_matched = _want(rows, n, contigs, starts, ends, 1, [0], [], 1, 0)
        assert len(want_runs) > engine.FIND_FIRST_CAP
        assert np.array_equal(runs, want_runs) and np.array_equal(matched.astype(np.int64), want_matched)
        total = len(want_runs)
        want_nruns = np.bincount(want_runs[:, 0], minlength=3)
        for cap, filled in [(total - 1, False), (total, True), (0, False)]:
            rs, re = np.full(total, 0xDEADBEEF, np.uint32), np.full(total, 0xDEADBEEF, np.uint32)
            code, got_total, nruns, m = _raw(res, contigs, starts, ends, hw, None, 1, 0, cap, rs if cap else None, re if cap else None)
            assert code == 0 and got_total == total, (cap, code, got_total)
            assert np.array_equal(nruns.astype(np.int64), want_nruns) and np.array_equal(m.astype(np.int64), want_matched)
            if filled:
                assert np.array_equal(rs, want_runs[:, 1]) and np.array_equal(re, want_runs[:, 2])
            else:
                assert (rs == 0xDEADBEEF).all() and (re == 0xDEADBEEF).all()
        # a NULL mask is the empty set: H empty and min_have 0, L empty -> every row, one run per window
        rs, re = np.zeros(3, np.uint32), np.zeros(3, np.uint32)
        code, got_total, nruns, m = _raw(res, contigs, starts, ends, None, None, 0, 0, 3, rs, re)
        assert code == 0 and got_total == 3 and rs.tolist() == starts and re.tolist() == ends
        assert m.tolist() == [e - s for s, e in zip(starts, ends)]
        # counts alone
        nruns, m = res.find_counts(contigs, starts, ends, hw, None, 1, 0)
        assert np.array_equal(nruns.astype(np.int64), want_nruns) and np.array_equal(m.astype(np.int64), want_matched)
    finally:
        res.close()


def test_refused_calls(ctx):
    """test_limit_and_rows_past_the_contig's cases: each is PG_E_INVALID before anything is launched"""
    from panagram_amd._lib import PanagramHipError
    res = rc.container(ctx, K, 4097, [300], colsums=False)
    try:
        with pytest.raises(PanagramHipError, match="1 to 4096") as ei:
            res.find_runs([0], [0], [300], None, None, 0, 0)
        assert ei.value.code == PG_E_INVALID
    finally:
        res.close()
    n = 12
    rows = [rc.dense(300, n, 2), rc.dense(50, n, 3)]
    res = rc.container(ctx, K, n, [300, 50], colsums=False)
    try:
        rc.plant(res, rows, poison=0xFF)
        res.rows_epilogue()
        hw, lw = rc.words_of(n, [1]), rc.words_of(n, [2])
        for contigs, starts, ends, stride, msg in [
                ([1], [0], [51], 1, "window 0: sampled row 50 (x 1) past the 50 rows of contig 1"),
                ([0], [0], [101], 3, "window 0: sampled row 100 (x 3) past the 300 rows of contig 0"),
                ([0, 1], [0, 40], [300, 60], 1, "window 1: sampled row 59 (x 1) past the 50 rows of contig 1"),
                ([2], [0], [1], 1, "window 0: contig 2 out of range"),
                ([0], [9], [8], 1, "window 0: start 9 past end 8"),
                ([0], [0], [10], 0, "pg_result_find_runs: stride must be >= 1"),
                ([2], [0], [10], 0, "pg_result_find_runs: stride must be >= 1")]:
            with pytest.raises(PanagramHipError) as ei:
                res.find_runs(contigs, starts, ends, hw, lw, 1, 0, step=1, stride=stride)
            assert ei.value.code == PG_E_INVALID and str(ei.value).endswith(msg), (str(ei.value), msg)
        with pytest.raises(PanagramHipError, match="step must be 1") as ei:
            res.find_runs([0], [0], [10], hw, lw, 1, 0, step=7, stride=0)
        assert ei.value.code == PG_E_INVALID
        # the last sampled rows that do fit
        for contigs, starts, ends, stride in [([0, 1], [0, 0], [300, 50], 1), ([0, 1], [0, 0], [100, 17], 3)]:
            runs, matched = res.find_runs(contigs, starts, ends, hw, lw, 1, 0, step=1, stride=stride)
            want_runs, want_matched = _want(rows, n, contigs, starts, ends, stride, [1], [2], 1, 0)
            assert np.array_equal(runs, want_runs) and np.array_equal(matched.astype(np.int64), want_matched)
    finally:
        res.close()
