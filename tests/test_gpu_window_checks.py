"""GPU: what the host checks of pg_result_bin_colsums, pg_result_pair_counts and pg_result_window_stats refuse, in which
words, and what they let through (panagram_amd/csrc: check_step in pg_api.hip, check_window_call, check_rows_readable and
gather_windows in pg_api_query.hip).  The two
first share their checks and differ in one noun; pg_result_window_stats clamps a window at its contig's end where they
refuse it.  The messages below were written down from the entry points as they stood before they shared those helpers.

Every check runs on the host before any launch: a rows container (tests/rows_craft.py) of N = 12 over contigs of 300 and
50 rows is enough, and only the small valid calls reach the device.  Their answers are those of tests/pairs_ref.py,
rows_craft.ref_bin_colsums and oracle.pyoracle.window_stats."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import rows_craft as rc
from tests.pairs_ref import ref_pair_counts

pytestmark = pytest.mark.gpu

K = 21
N = 12
NKS = [300, 50]
PG_E_INVALID = -1
STEP_MSG = "step must be 1 or the result's low-resolution step (100; 100 is accepted as its alias)"
NOUN = {"bin_colsums": "bin", "pair_counts": "window"}
CALLS = sorted(NOUN)

# (contigs, starts, ends, stride) -> what follows "<noun> " in the message
REFUSED = [
    ([2], [0], [1], 1, "0: contig 2 out of range"),
    ([0, 2], [0, 0], [10, 1], 1, "1: contig 2 out of range"),
    ([0], [9], [8], 1, "0: start 9 past end 8"),
    ([1, 0], [0, 9], [50, 8], 1, "1: start 9 past end 8"),
    ([1], [0], [51], 1, "0: sampled row 50 (x 1) past the 50 rows of contig 1"),
    ([0], [0], [101], 3, "0: sampled row 100 (x 3) past the 300 rows of contig 0"),
    ([0, 1], [0, 40], [300, 60], 1, "1: sampled row 59 (x 1) past the 50 rows of contig 1"),
    ([0, 1, 1], [0, 0, 0], [100, 18, 17], 3, "1: sampled row 17 (x 3) past the 50 rows of contig 1"),
]


@pytest.fixture(scope="module")
def planted(ctx):
    rows = [rc.dense(NKS[0], N, 2), rc.dense(NKS[1], N, 3)]
    res = rc.container(ctx, K, N, NKS, colsums=False)
    try:
        rc.plant(res, rows)
        res.rows_epilogue()
        yield res, rows
    finally:
        res.close()


def _refused(call, message):
    from panagram_amd._lib import PanagramHipError
    with pytest.raises(PanagramHipError) as ei:
        call()
    assert ei.value.code == PG_E_INVALID
    assert str(ei.value) == f"libpanagram_hip error {PG_E_INVALID}: {message}"


def _valid_calls_give_the_reference(res, rows):
    """the last sampled rows that do fit, at stride 1 and 3, from all three calls"""
    got = res.pair_counts([0, 1], [0, 0], [100, 50], step=1, stride=1)
    assert np.array_equal(got[0].astype(np.int64), ref_pair_counts(rows[0], N, 0, 100, 1))
    assert np.array_equal(got[1].astype(np.int64), ref_pair_counts(rows[1], N, 0, 50, 1))
    got = res.pair_counts([0], [0], [100], step=1, stride=3)
    assert np.array_equal(got[0].astype(np.int64), ref_pair_counts(rows[0], N, 0, 100, 3))
    for stride, s, e in [(1, [250, 0], [300, 7]), (3, [0, 99], [100, 100])]:
        cs, kept = res.bin_colsums([0, 0], s, e, step=1, stride=stride)
        want_cs, want_kept = rc.ref_bin_colsums(rows[0], N, s, e, stride, None, False)
        assert np.array_equal(cs.astype(np.int64), want_cs) and np.array_equal(kept.astype(np.int64), want_kept)
    cs, kept = res.bin_colsums([1], [0], [17], step=1, stride=3)  # (sampled row 16 = row 48 of 50)
    want_cs, want_kept = rc.ref_bin_colsums(rows[1], N, [0], [17], 3, None, False)
    assert np.array_equal(cs.astype(np.int64), want_cs) and np.array_equal(kept.astype(np.int64), want_kept)
    starts, ends = np.array([0, 290], np.uint64), np.array([300, 300], np.uint64)
    h, cs = res.window_stats(0, starts, ends)
    want_h, want_cs = po.window_stats(rows[0], N, starts, ends)
    assert np.array_equal(h.astype(np.int64), want_h) and np.array_equal(cs.astype(np.int64), want_cs)


@pytest.mark.parametrize("name", CALLS)
def test_windows_outside_their_contig_are_refused_by_name_and_number(planted, name):
    """contig index 2, start past end, a last sampled row one past the contig at stride 1 and 3: PG_E_INVALID, the call's
    noun, and the number of the FIRST offending item when it is not item 0; the next valid calls answer as ever"""
    res, rows = planted
    for contigs, starts, ends, stride, tail in REFUSED:
        _refused(lambda: getattr(res, name)(contigs, starts, ends, step=1, stride=stride), f"{NOUN[name]} {tail}")
    _valid_calls_give_the_reference(res, rows)


@pytest.mark.parametrize("name", CALLS)
def test_stride_and_step_are_refused_before_the_windows(planted, name):
    """stride 0 and a step that is none of 1, 100 and the result's low-resolution step (100 here) — also when a window of
    the same call is out of range: the step is looked at first, then the stride, then the windows"""
    res, rows = planted
    call = getattr(res, name)
    _refused(lambda: call([0], [0], [10], step=1, stride=0), f"pg_result_{name}: stride must be >= 1")
    _refused(lambda: call([0], [0], [10], step=7, stride=1), STEP_MSG)
    _refused(lambda: call([2], [0], [10], step=7, stride=0), STEP_MSG)
    _refused(lambda: call([2], [0], [10], step=1, stride=0), f"pg_result_{name}: stride must be >= 1")
    _refused(lambda: call([], [], [], step=7, stride=1), STEP_MSG)
    _valid_calls_give_the_reference(res, rows)


def test_window_stats_refuses_contig_and_step_and_clamps_windows(planted):
    """pg_result_window_stats: a contig index and a step out of range are refused (the contig first); a window that runs
    past its contig is ACCEPTED and equals the same window cut at the contig's end — here it must not turn into the
    refusal the other two calls make"""
    res, rows = planted
    _refused(lambda: res.window_stats(2, [0], [1]), "contig 2 out of range")
    _refused(lambda: res.window_stats(0, [0], [1], step=7), STEP_MSG)
    _refused(lambda: res.window_stats(2, [0], [1], step=7), "contig 2 out of range")
    for ci, nk in enumerate(NKS):
        past = (np.array([nk - 10, 0, nk, nk + 5], np.uint64), np.array([nk + 100, nk + 1, nk + 7, nk + 9], np.uint64))
        cut = (np.array([nk - 10, 0, nk, nk], np.uint64), np.array([nk, nk, nk, nk], np.uint64))
        h, cs = res.window_stats(ci, *past)
        h_cut, cs_cut = res.window_stats(ci, *cut)
        assert np.array_equal(h, h_cut) and np.array_equal(cs, cs_cut)
        want_h, want_cs = po.window_stats(rows[ci], N, *cut)
        assert np.array_equal(h.astype(np.int64), want_h) and np.array_equal(cs.astype(np.int64), want_cs)
        assert h[0].sum() == 10 and h[1].sum() == nk and not h[2:].any()
    _valid_calls_give_the_reference(res, rows)


def test_no_window_is_an_empty_answer(planted):
    res, _ = planted
    for stride in (1, 3):
        pairs = res.pair_counts([], [], [], step=1, stride=stride)
        assert pairs.shape == (0, N, N) and pairs.dtype == np.uint64
        cs, kept = res.bin_colsums([], [], [], step=1, stride=stride)
        assert cs.shape == (0, N) and kept.shape == (0,) and cs.dtype == kept.dtype == np.uint64
    h, cs = res.window_stats(0, [], [])
    assert h.shape == (0, N + 1) and cs.shape == (0, N)
    h, cs = res.window_stats(1, [], [], step=100, colsums=False)
    assert h.shape == (0, N + 1) and cs is None
