"""GPU: k_absence_runs (panagram_amd/csrc/pg_gaps.hip) and the stitch of its chunk edges on rows PLANTED into a rows container
(tests/rows_craft.py), every byte that is not a row byte holding 0xFF and the bits past N in a row's last byte set.  Every
result — spectrum, absent rows, open runs, the emitted records and their order — is exactly equal to the numpy restatement
(tests/gaps_ref.py, tied on the CPU to a hand-written loop: tests/test_gaps_cpu.py).

Which kernel runs for which N: N <= 128 k_absence_runs<4, 1, .> (the row's words in registers), N <= 256 <0, 1, .>, beyond
<0, 2, .> (two columns per thread); the spectrum's atomics go to LDS while N * (maxlen + 1) <= 6144 (N = 512 at maxlen 21
and every N but 1 at maxlen 4096 go to HBM).  A wave takes 64 sampled rows, a tile is 256, a workgroup's chunk
engine.GAPS_CHUNK; chunks count from their window's first sampled row, so a window's start moves every border."""
import ctypes as C

import numpy as np
import pytest

from tests import gaps_ref as gr
from tests import rows_craft as rc

pytestmark = pytest.mark.gpu

K = 21
GAPS_N = [1, 7, 8, 9, 32, 33, 64, 65, 128, 129, 257, 512]
PG_E_INVALID = -1
A0 = 700  # first row of column 0's planted run


def _chunk():
    from panagram_amd import engine
    return engine.GAPS_CHUNK


def _nks():
    return [5 * _chunk() + 77, 1111]


def _run_lengths():
    ch = _chunk()
    return [1, 63, 64, 65, 255, 256, 257, ch, ch + 1, 2 * ch + 3]  # (the last: a chunk that is absent throughout)


def _start(g):
    return A0 + 11 * ((g // 4) % 5) + (g % 4 == 1)


_BACKGROUND = {}


def _background(n):
    """(bits of contig 0 without the planted runs, contig 1's rows), made once per N: the columns g % 4 >= 2 do not depend on
    the runs' length"""
    if n not in _BACKGROUND:
        nk0, nk1 = _nks()
        bits = np.ones((nk0, n), np.uint8)
        rng = np.random.default_rng(1000 + n)
        for g in range(2, n, 4):
            bits[:, g] = rng.random(nk0) < 0.3
        for g in range(3, n, 4):
            bits[:, g] = (np.arange(nk0) % 5000) == 4999 - (g % 7)
        for g in range(1, n, 4):
            bits[nk0 - 500::2, g] = 0
        _BACKGROUND.clear()  # (one N at a time: the tests come N by N)
        _BACKGROUND[n] = (bits, rc.with_pad_bits(rc.dense(nk1, n, 7 + n), n))
    return _BACKGROUND[n]


def planted_runs(n, length):
    """contig 0, by column g % 4: 0 — present but for two runs of `length` rows, the first from row _start(g), the second 1 to 3
    present rows behind it; 1 — the same one row further on, and single absent rows over the last 500 rows; 2 — seven rows
    in ten absent (runs of every small length); 3 — absent but for one row in 5000 (chunks absent throughout, runs longer
    than a chunk).  Neighbouring columns differ.  contig 1: dense."""
    nk0, _ = _nks()
    background, contig1 = _background(n)
    bits = background.copy()
    for g in range(n):
        if g % 4 <= 1:
            a = _start(g)
            bits[a:a + length, g] = 0
            a2 = a + length + 1 + (g // 4) % 3
            if a2 + length < nk0 - 600:
                bits[a2:a2 + length, g] = 0
    return [rc.with_pad_bits(rc.pack(bits), n), contig1]


def border_windows(length):
    """(contigs, starts, ends): contig 0 whole; for the word, the tile and the chunk, windows whose start puts column 0's
    first run (rows [A0, A0 + length)) so that it STARTS on the unit's first row, ENDS on its last row, and STRADDLES a border;
    a window inside the run (absent throughout for column 0), one that starts inside the first run and ends inside the second;
    an empty window, a window of one row, contig 1 whole — twice — and one row of it"""
    nk0, nk1 = _nks()
    ch = _chunk()
    w = [(0, 0, nk0), (0, 5, 5), (0, A0, A0 + 1), (1, 0, nk1), (1, 0, nk1), (1, 5, 6)]
    for unit in (64, 256, ch):
        far = min(nk0, A0 + 2 * length + 2 * unit + 600)
        w += [(0, A0 % unit, far), (0, (A0 + length) % unit, far), (0, (A0 + max(1, length // 2)) % unit, far)]
    if length > 2:
        w.append((0, A0 + 1, A0 + length - 1))
    w.append((0, A0 + length // 2, min(nk0, A0 + length + 1 + length // 2 + 1)))
    c, s, e = (np.array(x) for x in zip(*w))
    return c.astype(np.uint32), s.astype(np.uint64), e.astype(np.uint64)


def _check(res, rows, n, windows, tag, stride=1, step=1, cols=None, maxlen=21, min_len=1, max_len=0, ref_rows=None):
    contigs, starts, ends = windows
    sel = None if cols is None else rc.words_of(n, cols)
    got = res.absence_runs(contigs, starts, ends, sel, maxlen, min_len, max_len, step=step, stride=stride)
    want = gr.ref_absence_runs(rows if ref_rows is None else ref_rows, n, contigs, starts, ends, stride, maxlen, min_len, max_len, cols)
    assert got[0].dtype == np.int64 and got[0].shape == want[0].shape, (tag, n, got[0].shape, want[0].shape)
    for a, b, what in zip(got, want, ("runs", "hist", "absent", "edges")):
        assert np.array_equal(a.astype(np.int64), b), (tag, n, stride, what)
    return got


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


@pytest.mark.parametrize("planted", GAPS_N, indirect=True)
def test_run_lengths_on_every_word_tile_and_chunk_border(planted):
    res, n = planted
    for length in _run_lengths():
        rows = planted_runs(n, length)
        rc.plant(res, rows, poison=0xFF)
        windows = border_windows(length)
        runs, hist, absent, edges = _check(res, rows, n, windows, f"length {length}")
        # column 0's first run is closed in every window that holds it whole with a row on both sides: the whole contig does
        assert (runs[(runs[:, 0] == 0) & (runs[:, 1] == 0) & (runs[:, 2] == A0)][:, 3] == length).all()
        assert len(runs[(runs[:, 0] == 0) & (runs[:, 1] == 0) & (runs[:, 2] == A0)]) == 1
        if length > 2:  # the window inside the run: no closed run, both edges the window's rows
            i = len(windows[0]) - 2
            assert edges[i, 0].tolist() == [length - 2, length - 2] and absent[i, 0] == length - 2 and not hist[i, 0].any()


@pytest.mark.parametrize("planted", GAPS_N, indirect=True)
def test_windows_strides_and_the_low_resolution_rows(planted):
    """tests/test_gpu_find.py's window set (empty, one row, lengths around 64 and 256 from odd starts, a chunk and a bit, exactly
    one and two chunks, both contigs) at stride 1, 3 and 100 over rows seven in ten absent, then rows absent and rows present
    throughout; the low-resolution rows of the same container at stride 1 and 2; the same call twice"""
    from panagram_amd import engine
    from tests.test_gpu_find import windows as find_windows
    assert engine.GAPS_CHUNK == engine.FIND_CHUNK  # (the window set aims at find's chunk edges)
    res, n = planted
    nks = _nks()
    rows = [rc.with_pad_bits(rc.pack(np.random.default_rng(50 + n + i).random((nk, n)) < 0.3), n) for i, nk in enumerate(nks)]
    rc.plant(res, rows, poison=0xFF)
    res.rows_epilogue()
    for stride in (1, 3, 100):
        a = _check(res, rows, n, find_windows(nks, stride), "dense", stride=stride)
        assert stride != 1 or len(a[0]) > 1000
    low = [r[::100] for r in rows]
    nlow = [len(r) for r in low]
    for stride in (1, 2):
        ns = [(m - 1) // stride + 1 for m in nlow]
        w = (np.array([0, 1, 0, 0], np.uint32), np.array([0, 0, 3, ns[0] - 1], np.uint64), np.array([ns[0], ns[1], ns[0] - 2, ns[0]], np.uint64))
        _check(res, rows, n, w, "low resolution", stride=stride, step=100, ref_rows=low)
    w = find_windows(nks, 1)
    a = res.absence_runs(*w, None, 21, 2, 0)
    b = res.absence_runs(*w, None, 21, 2, 0)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a[0]) > 100
    for name, gen in (("absent throughout", rc.zeros), ("present throughout", rc.ones)):
        rows = [rc.with_pad_bits(gen(nk, n), n) for nk in nks]
        rc.plant(res, rows, poison=0xFF)
        runs, hist, absent, edges = _check(res, rows, n, w, name)
        assert len(runs) == 0 and not hist.any()
        assert np.array_equal(edges[:, :, 0], edges[:, :, 1]) and np.array_equal(absent, edges[:, :, 0])
        assert np.array_equal(absent[:, 0], (w[2] - w[1]) if gen is rc.zeros else np.zeros(len(w[0]), np.uint64))


@pytest.mark.parametrize("planted", GAPS_N, indirect=True)
def test_selection_spectrum_cap_and_length_filter(planted):
    res, n = planted
    rows = planted_runs(n, 65)
    rc.plant(res, rows, poison=0xFF)
    windows = border_windows(65)
    subset = sorted({0, n - 1} | set(range(2, n, 3)))
    for cols in (None, subset, [n - 1]):
        for maxlen in (1, 21, 4096):
            runs, hist, absent, edges = _check(res, rows, n, windows, f"cols {cols} maxlen {maxlen}", cols=cols, maxlen=maxlen)
            if cols is not None:
                out = sorted(set(range(n)) - set(cols))
                assert not hist[:, out].any() and not absent[:, out].any() and not edges[:, out].any()
                assert not np.isin(runs[:, 1], out).any()
    for min_len, max_len in [(2, 5), (65, 65), (66, 0), (5, 3), (1, 1)]:
        runs, _, _, _ = _check(res, rows, n, windows, f"min_len {min_len} max_len {max_len}", cols=subset, min_len=min_len, max_len=max_len)
        assert (min_len, max_len) != (5, 3) or len(runs) == 0
        assert (min_len, max_len) != (65, 65) or len(runs) > 0
    # without emission: the tables alone
    got = res.absence_runs(*windows, None, 21, emit=False)
    want = gr.ref_absence_runs(rows, n, *windows, 1, 21)
    assert got[0].shape == (0, 4) and all(np.array_equal(a.astype(np.int64), b) for a, b in zip(got[1:], want[1:]))


def _raw(res, contigs, starts, ends, maxlen, min_len, max_len, cap, arrays, sel=None, stride=1, step=1):
    contigs, starts, ends = np.asarray(contigs, np.uint32), np.asarray(starts, np.uint64), np.asarray(ends, np.uint64)
    n, N = len(contigs), res.ngenomes
    hist, absent = np.full((n, N, maxlen + 1), 77, np.uint64), np.full((n, N), 77, np.uint64)
    edges, nruns, total = np.full((n, N, 2), 77, np.uint64), np.full(n, 77, np.uint64), C.c_uint64(12345)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rg, rs, rr = arrays if cap else (None, None, None)
    code = res._lib.pg_result_absence_runs(res._h, step, stride, n, vp(contigs), vp(starts), vp(ends), vp(sel), maxlen, min_len,
                                           max_len, cap, vp(rg), vp(rs), vp(rr), vp(hist), vp(absent), vp(edges), vp(nruns),
                                           C.byref(total))
    return code, total.value, hist, absent, edges, nruns


@pytest.mark.parametrize("n", [8, 130])
def test_capacity(ctx, n):
    """more runs than engine.GAPS_FIRST_CAP: absence_runs makes its second call; at the ABI, cap = total - 1 leaves the run
    arrays untouched and still fills the tables, cap = total fills them, cap = 0 takes NULL arrays"""
    from panagram_amd import engine
    nks = _nks()
    rows = [rc.checker(nk, n) for nk in nks]
    res = rc.container(ctx, K, n, nks, colsums=False)
    try:
        rc.plant(res, rows, poison=0xFF)
        res.rows_epilogue()
        contigs, starts, ends = [0, 1, 0], [0, 0, 1001], [nks[0], nks[1], 3003]
        want = gr.ref_absence_runs(rows, n, contigs, starts, ends, 1, 4)
        total = len(want[0])
        assert total > engine.GAPS_FIRST_CAP
        got = res.absence_runs(contigs, starts, ends, None, 4)
        assert all(np.array_equal(a.astype(np.int64), b) for a, b in zip(got, want))
        want_nruns = np.bincount(want[0][:, 0], minlength=3)
        for cap, filled in [(total - 1, False), (total, True), (0, False)]:
            arrays = [np.full(total, 0xDEADBEEF, np.uint32) for _ in range(3)]
            code, got_total, hist, absent, edges, nruns = _raw(res, contigs, starts, ends, 4, 1, 0, cap, arrays)
            assert code == 0 and got_total == total, (cap, code, got_total)
            assert np.array_equal(nruns.astype(np.int64), want_nruns)
            for a, b in zip((hist, absent, edges), want[1:]):
                assert np.array_equal(a.astype(np.int64), b), cap
            if filled:
                assert all(np.array_equal(a, want[0][:, 1 + i]) for i, a in enumerate(arrays))
            else:
                assert all((a == 0xDEADBEEF).all() for a in arrays)
        # no window: nothing to write, a total of 0
        code, got_total, *_ = _raw(res, [], [], [], 4, 1, 0, 0, None)
        assert code == 0 and got_total == 0
        runs, hist, absent, edges = res.absence_runs([], [], [])
        assert runs.shape == (0, 4) and hist.shape == (0, n, 85) and absent.shape == (0, n) and edges.shape == (0, n, 2)
    finally:
        res.close()


def test_refused_calls(ctx):
    """each is PG_E_INVALID before anything is launched, and leaves the caller's arrays alone"""
    from panagram_amd._lib import PanagramHipError
    res = rc.container(ctx, K, 513, [300], colsums=False)
    try:
        with pytest.raises(PanagramHipError, match="1 to 512") as ei:
            res.absence_runs([0], [0], [300])
        assert ei.value.code == PG_E_INVALID
    finally:
        res.close()
    n = 12
    rows = [rc.dense(300, n, 2), rc.dense(50, n, 3)]
    res = rc.container(ctx, K, n, [300, 50], colsums=False)
    try:
        rc.plant(res, rows, poison=0xFF)
        res.rows_epilogue()
        for kw, msg in [(dict(maxlen=0), "maxlen = 0 (the spectrum takes 1 to 4096)"), (dict(maxlen=4097), "maxlen = 4097 (the spectrum takes 1 to 4096)"),
                        (dict(min_len=0), "min_len must be >= 1")]:
            with pytest.raises(PanagramHipError) as ei:
                res.absence_runs([0], [0], [300], **kw)
            assert ei.value.code == PG_E_INVALID and str(ei.value).endswith(msg), (str(ei.value), msg)
        for contigs, starts, ends, stride, msg in [
                ([1], [0], [51], 1, "window 0: sampled row 50 (x 1) past the 50 rows of contig 1"),
                ([0], [0], [101], 3, "window 0: sampled row 100 (x 3) past the 300 rows of contig 0"),
                ([0, 1], [0, 40], [300, 60], 1, "window 1: sampled row 59 (x 1) past the 50 rows of contig 1"),
                ([2], [0], [1], 1, "window 0: contig 2 out of range"),
                ([0], [9], [8], 1, "window 0: start 9 past end 8"),
                ([0], [0], [10], 0, "pg_result_absence_runs: stride must be >= 1")]:
            with pytest.raises(PanagramHipError) as ei:
                res.absence_runs(contigs, starts, ends, stride=stride)
            assert ei.value.code == PG_E_INVALID and str(ei.value).endswith(msg), (str(ei.value), msg)
        with pytest.raises(PanagramHipError, match="step must be 1") as ei:
            res.absence_runs([0], [0], [10], step=7)
        assert ei.value.code == PG_E_INVALID
        code, total, hist, absent, edges, nruns = _raw(res, [0], [0], [300], 4097, 1, 0, 0, None)
        assert code == PG_E_INVALID and all((a == 77).all() for a in (hist, absent, edges, nruns))
        # the last sampled rows that do fit
        for contigs, starts, ends, stride in [([0, 1], [0, 0], [300, 50], 1), ([0, 1], [0, 0], [100, 17], 3)]:
            got = res.absence_runs(contigs, starts, ends, stride=stride)
            want = gr.ref_absence_runs(rows, n, contigs, starts, ends, stride, 84)
            assert all(np.array_equal(a.astype(np.int64), b) for a, b in zip(got, want))
    finally:
        res.close()


@pytest.mark.parametrize("n, density", [(33, 0.5), (9, 0.05), (130, 0.9)])
def test_every_absent_row_is_in_exactly_one_run(ctx, n, density):
    """on random rows: the rows of the closed runs below maxlen (from the spectrum), of the closed runs of maxlen rows and more
    (from the emitted records) and of the open runs add up to the absent rows, per window and genome"""
    from panagram_amd import gaps
    nks = _nks()
    rows = [rc.pack(np.random.default_rng(90 + n + i).random((nk, n)) < density) for i, nk in enumerate(nks)]
    res = rc.container(ctx, K, n, nks, colsums=False)
    try:
        rc.plant(res, rows, poison=0xFF)
        res.rows_epilogue()
        contigs, starts, ends = [0, 1, 0], [0, 3, 4000], [nks[0], nks[1] - 1, 4000 + 2 * _chunk()]
        maxlen = 6
        runs, hist, absent, edges = res.absence_runs(contigs, starts, ends, None, maxlen, min_len=maxlen)
        hist, absent = hist.astype(np.int64), absent.astype(np.int64)
        short = (hist[:, :, :maxlen] * np.arange(maxlen)).sum(axis=2)
        capped = np.zeros_like(absent)
        np.add.at(capped, (runs[:, 0], runs[:, 1]), runs[:, 3])
        assert (runs[:, 3] >= maxlen).all() and np.array_equal(np.bincount(runs[:, 0] * n + runs[:, 1], minlength=3 * n).reshape(3, n), hist[:, :, maxlen])
        opened = np.stack([gaps.open_rows(edges[i], ends[i] - starts[i]) for i in range(3)])
        assert np.array_equal(short + capped + opened, absent) and absent.sum() > 0
    finally:
        res.close()
