"""GPU: k_presence_profile (panagram_amd/csrc/pg_profile.hip) and the stitch of its chunk partials on rows PLANTED into a rows
container (tests/rows_craft.py), every byte that is not a row byte holding 0xFF and the bits past N in a row's last byte set.
Every field — hits, runs, longest, first, end, covered per window and genome, all and none per window — is exactly equal to the
numpy model (tests/search_ref.py, tied on the CPU to a loop that marks bases: tests/test_search_cpu.py).

Which kernel runs for which N: N <= 128 k_presence_profile<4, 1> (the row's words in registers), N <= 256 <0, 1>, beyond <0, 2>
(two columns per thread); rows of a whole number of 32-bit words are read as words, the others byte by byte.  A wave takes 64
rows, a tile is 256, a workgroup's chunk engine.PROFILE_CHUNK; chunks count from their window's first row.

The planted contig: per window length one window, every column a pattern of its own (pattern(), by column number; narrow rows
repeat the windows until every pattern has had a column), the windows apart by rows of ALL ONES and starting off the multiples of
64 — a row outside a window that leaked into it would show in every field."""
import ctypes as C

import numpy as np
import pytest

from tests import rows_craft as rc
from tests import search_ref as sr

pytestmark = pytest.mark.gpu

PROFILE_N = [1, 8, 9, 16, 24, 32, 33, 64, 65, 128, 130, 257, 512]
PROFILE_K = [1, 2, 21, 31, 32]
PG_E_INVALID = -1
GAPS = [1, 2, 19, 20, 21, 22, 29, 30, 31, 32, 33]  # k - 2, k - 1 and k (and k + 1) rows for every k of PROFILE_K
NPATTERNS = 14


def _chunk():
    from panagram_amd import engine
    return engine.PROFILE_CHUNK


def _lengths():
    ch = _chunk()
    # (the last: three chunks, the middle one whole, the outer two partly set — 2 ch + 1 leaves the third chunk one row)
    return [1, 63, 64, 65, 255, 256, 257, ch - 1, ch, ch + 1, 2 * ch + 1, 2 * ch + 130]


def pattern(pid, v, n, rng):
    """column pattern `pid`, variant `v`, of a window of n rows: 0 / 1 per row"""
    ch = _chunk()
    p = np.zeros(n, np.uint8)
    at = np.arange(n)
    if pid == 0:    # all set
        p[:] = 1
    elif pid == 1:  # none set
        pass
    elif pid == 2:  # alternating
        p[:] = (at + v) % 2
    elif pid == 3:  # a single set row: at 0, 63, 64, the chunk's last row, the next chunk's first, the window's last
        where = [r for r in (0, 63, 64, ch - 1, ch, n - 1) if r < n]
        p[where[v % len(where)]] = 1
    elif pid == 4:  # one run that straddles a word, a tile or a chunk edge
        edges = [e for e in (64, 256, ch, 2 * ch) if e < n] or [max(1, n // 2)]
        e = edges[v % len(edges)]
        p[max(0, e - 1 - (7 * v) % 50):min(n, e + 1 + (3 * v) % 40)] = 1
        p[0] = v & 1
    elif pid == 5:  # a run covering one whole chunk between two partly set ones
        if n > 2 * ch + 1:
            p[ch - 1 - v % 60:2 * ch + 1 + v % 50] = 1
            p[[3, 7]] = 1
        else:
            p[n // 3:max(n // 3 + 1, 2 * n // 3)] = 1
    elif pid == 6:  # gaps of k - 2, k - 1, k rows one after the other, inside words and across their edges
        p[:] = 1
        pos = 1 + v % 7
        for i in range(len(GAPS)):
            g = GAPS[(i + v) % len(GAPS)]
            if pos + g + 1 >= n:
                break
            p[pos:pos + g] = 0
            pos += g + 1 + (v + g) % 3
    elif pid == 7:  # one gap of k - 2, k - 1, k rows across the chunk edge (a shorter window: across its middle)
        p[:] = 1
        g = GAPS[v % len(GAPS)]
        c = ch if n > ch + g else n // 2
        lo = max(1, c - 1 - (v // len(GAPS)) % g)
        p[lo:min(n - 1, lo + g)] = 0
    elif pid in (8, 9):  # the longest run at the window's start / at its end
        m = min(n, 40 + v)
        p[:m] = 1
        p[m + 1::4] = 1
        p[m + 2::4] = 1
        if pid == 9:
            p = p[::-1].copy()
    elif pid == 10:  # the longest run cut by a chunk edge (a shorter window: by a word edge, or its middle)
        p[::5] = 1
        c = ch if n > ch else (64 if n > 64 else n // 2)
        p[max(0, c - 30 - v):min(n, c + 50 + v)] = 1
    elif pid == 11:
        p[:] = rng.random(n) < 0.5
    elif pid == 12:
        p[:] = rng.random(n) < 0.05
    else:
        p[:] = rng.random(n) < 0.95
    return p


_PLANTED = {}


def planted(n):
    """(rows of the one contig with their pad bits set, (contigs, starts, ends) of its windows), made once per N"""
    if n not in _PLANTED:
        rng = np.random.default_rng(4000 + n)
        parts, starts, ends, at = [], [], [], 0
        for rot in range(0, NPATTERNS, n):  # (narrow rows: the windows again, the patterns moved on by N)
            for length in _lengths():
                sep = 37 if (at + 37) % 64 else 38  # rows of all ones between the windows; no window starts on a multiple of 64
                parts.append(np.ones((sep, n), np.uint8))
                at += sep
                assert at % 64
                bits = np.stack([pattern((g + rot) % NPATTERNS, (g + rot) // NPATTERNS, length, rng) for g in range(n)], axis=1)
                parts.append(bits)
                starts.append(at)
                ends.append(at + length)
                at += length
        parts.append(np.ones((29, n), np.uint8))
        rows = rc.with_pad_bits(rc.pack(np.concatenate(parts)), n)
        _PLANTED.clear()  # (one N at a time: the tests come N by N)
        _PLANTED[n] = (rows, (np.zeros(len(starts), np.uint32), np.array(starts, np.uint64), np.array(ends, np.uint64)))
    return _PLANTED[n]


def _check(res, rows, n, k, windows, tag, cols=None):
    contigs, starts, ends = windows
    sel = None if cols is None else rc.words_of(n, cols)
    prof, allnone = res.presence_profile(contigs, starts, ends, sel)
    want = sr.ref_presence_profile(rows, n, k, contigs, starts, ends, cols)
    assert prof.dtype == np.uint32 and prof.shape == want[0].shape and allnone.dtype == np.uint32 and allnone.shape == want[1].shape
    for f, name in enumerate(sr.FIELDS):
        bad = np.argwhere(prof[:, :, f].astype(np.int64) != want[0][:, :, f])
        assert len(bad) == 0, (tag, n, k, name, [(int(i), int(g), int(ends[i] - starts[i]), int(prof[i, g, f]), int(want[0][i, g, f])) for i, g in bad[:5]])
    assert np.array_equal(allnone.astype(np.int64), want[1]), (tag, n, k, allnone[:5], want[1][:5])
    return prof.astype(np.int64), allnone.astype(np.int64)


def _container(ctx, k, n, rows_per_contig):
    res = rc.container(ctx, k, n, [len(r) for r in rows_per_contig], colsums=False)
    try:
        rc.plant(res, rows_per_contig, poison=0xFF)
        res.rows_epilogue()  # (a rows container is read once its statistics have been enqueued)
    except Exception:
        res.close()
        raise
    return res


@pytest.mark.parametrize("n", PROFILE_N)
def test_patterns_on_every_word_tile_and_chunk_border(ctx, n):
    rows, windows = planted(n)
    lengths = (windows[2] - windows[1]).astype(np.int64)
    for k in PROFILE_K:
        res = _container(ctx, k, n, [rows])
        try:
            prof, allnone = _check(res, [rows], n, k, windows, "patterns")
            if k == 21:  # a subset of the genomes — the others' outputs zero, all / none over the subset —, and no genome
                subset = sorted({0, n - 1} | set(range(2, n, 3)))
                part, _ = _check(res, [rows], n, k, windows, "subset", cols=subset)
                out = sorted(set(range(n)) - set(subset))
                assert not part[:, out].any() and np.array_equal(part[:, subset], prof[:, subset])
                none, _ = _check(res, [rows], n, k, windows, "no genome", cols=[])
                assert not none.any()
        finally:
            res.close()
        # what the patterns are there for, on the first block of windows (column g there holds pattern g)
        first = slice(0, len(_lengths()))
        assert (prof[first, 0, 0] == lengths[first]).all() and (prof[first, 0, 2] == lengths[first]).all()  # all set
        assert (prof[first, 0, 5] == lengths[first] + k - 1).all() and (prof[first, 0, 1] == 1).all()
        if n > 1:
            assert not prof[first, 1].any()  # none set
        if n == 1:
            assert np.array_equal(allnone[first, 0], lengths[first])


@pytest.mark.parametrize("n", [9, 64])
def test_many_short_windows_in_one_call(ctx, n):
    """3000 windows of 0 to 200 rows over three contigs, empty ones among them, in one call"""
    k = 21
    rng = np.random.default_rng(70 + n)
    nks = [5000, 333, 1]
    rows = [rc.with_pad_bits(rc.pack(rng.random((nk, n)) < d), n) for nk, d in zip(nks, (0.7, 0.3, 1.0))]
    contigs = rng.integers(0, 3, 3000).astype(np.uint32)
    contigs[:3] = [0, 1, 2]
    length = rng.integers(0, 201, 3000)
    length[5::17] = 0
    room = np.array(nks)[contigs]
    length = np.minimum(length, room)
    starts = (rng.random(3000) * (room - length + 1)).astype(np.uint64)
    ends = starts + length.astype(np.uint64)
    assert (length == 0).sum() > 100 and (length == 200).sum() > 3 and ends.max() <= 5000
    res = _container(ctx, k, n, rows)
    try:
        prof, _ = _check(res, rows, n, k, (contigs, starts, ends), "short windows")
        assert not prof[length == 0].any() and prof[length > 0, :, 0].sum() > 10000
        # no window at all
        prof, allnone = res.presence_profile([], [], [])
        assert prof.shape == (0, n, 6) and allnone.shape == (0, 2)
    finally:
        res.close()


def _raw(res, contigs, starts, ends, sel=None, null=()):
    """the entry point itself: (code, profile, rows), the outputs filled with 77 before the call"""
    contigs, starts, ends = np.asarray(contigs, np.uint32), np.asarray(starts, np.uint64), np.asarray(ends, np.uint64)
    n, N = len(contigs), res.ngenomes
    prof, allnone = np.full((n, N, 6), 77, np.uint32), np.full((n, 2), 77, np.uint32)
    args = {"contig": contigs, "starts": starts, "ends": ends, "select": sel, "profile": prof, "rows": allnone}
    vp = lambda name: None if name in null or args[name] is None else args[name].ctypes.data_as(C.c_void_p)
    code = res._lib.pg_result_presence_profile(None if "result" in null else res._h, n, vp("contig"), vp("starts"), vp("ends"),
                                               vp("select"), vp("profile"), vp("rows"))
    return code, prof, allnone


def test_refused_calls(ctx):
    """each is PG_E_INVALID before anything is launched, leaves the caller's arrays alone and the context usable"""
    from panagram_amd._lib import PanagramHipError
    k, n = 21, 12
    rows = [rc.dense(300, n, 2), rc.dense(50, n, 3)]
    res = _container(ctx, k, n, rows)
    wide = rc.container(ctx, k, 513, [300], colsums=False)
    try:
        def still_works():
            _check(res, rows, n, k, ([0, 1], np.array([0, 0], np.uint64), np.array([300, 50], np.uint64)), "after a refusal")

        with pytest.raises(PanagramHipError, match="1 to 512") as ei:
            wide.presence_profile([0], [0], [300])
        assert ei.value.code == PG_E_INVALID
        still_works()
        for contigs, starts, ends, msg in [
                ([1], [0], [51], "window 0: sampled row 50 (x 1) past the 50 rows of contig 1"),
                ([0, 1], [0, 40], [300, 60], "window 1: sampled row 59 (x 1) past the 50 rows of contig 1"),
                ([2], [0], [1], "window 0: contig 2 out of range"),
                ([0], [9], [8], "window 0: start 9 past end 8"),
                ([0, 0], [0, 0], [300, 1 << 32], f"window 1: 4294967296 rows of k = {k} are 4294967316 bases (below 2^32 per window)"),
                ([0], [5], [(1 << 32) - k + 6], f"window 0: {(1 << 32) - k + 1} rows of k = {k} are 4294967296 bases (below 2^32 per window)")]:
            with pytest.raises(PanagramHipError) as ei:
                res.presence_profile(contigs, starts, ends)
            assert ei.value.code == PG_E_INVALID and str(ei.value).endswith(msg), (str(ei.value), msg)
            code, prof, allnone = _raw(res, contigs, starts, ends)
            assert code == PG_E_INVALID and (prof == 77).all() and (allnone == 77).all()
            still_works()
        for null in ("result", "contig", "starts", "ends", "profile", "rows"):
            code, prof, allnone = _raw(res, [0], [0], [300], null=(null,))
            assert code == PG_E_INVALID and (prof == 77).all() and (allnone == 77).all(), null
            assert "NULL argument" in res._lib.pg_last_error().decode()
        still_works()
        # a NULL selection is every genome; the last rows that do fit
        code, prof, allnone = _raw(res, [0, 1], [299, 49], [300, 50])
        want = sr.ref_presence_profile(rows, n, k, [0, 1], [299, 49], [300, 50])
        assert code == 0 and np.array_equal(prof, want[0]) and np.array_equal(allnone, want[1])
    finally:
        wide.close()
        res.close()


@pytest.mark.parametrize("n", [8, 130])
def test_cross_check_on_the_gpus_own_absence_runs(ctx, n):
    """the same windows through k_absence_runs with maxlen >= k: hits = rows - absent, first / end from the open runs, and both
    identities — covered = hits + sum of min(k - 1, L) + (k - 1 if hits), runs = #L + (1 if hits) — with L from its spectrum of
    closed runs"""
    k, maxlen = 21, 40
    rows, windows = planted(n)
    res = _container(ctx, k, n, [rows])
    try:
        prof, allnone = res.presence_profile(*windows)
        _, hist, absent, edges = res.absence_runs(*windows, None, maxlen, emit=False)
    finally:
        res.close()
    prof, hist, absent, edges = prof.astype(np.int64), hist.astype(np.int64), absent.astype(np.int64), edges.astype(np.int64)
    length = (windows[2] - windows[1]).astype(np.int64)[:, None]
    hits = prof[:, :, 0]
    some = hits > 0
    assert np.array_equal(hits, length - absent) and some.any() and (~some).any()
    assert np.array_equal(prof[:, :, 1], hist.sum(axis=2) + some)
    clipped = (hist * np.minimum(np.arange(maxlen + 1), k - 1)).sum(axis=2)
    assert np.array_equal(prof[:, :, 5], hits + clipped + (k - 1) * some)
    assert np.array_equal(prof[:, :, 3][some], edges[:, :, 0][some]) and np.array_equal(prof[:, :, 4][some], (length - edges[:, :, 1])[some])
    assert not prof[~some].any() and (hist[:, :, k - 2:k + 1].sum(axis=(0, 1)) > 0).all()  # gaps of k - 2, k - 1 and k rows occurred
