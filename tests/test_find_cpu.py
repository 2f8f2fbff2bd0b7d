"""CPU: the host side of the pattern search — the numpy restatement of k_find_runs (tests/find_ref.py) against
scripts/query_index.py's literal expression and hand-written cases, and panagram_amd/find.py: rule_words, merge_runs,
join_pieces."""
import os
import re

import numpy as np
import pytest

from panagram_amd import find
from tests import rows_craft as rc
from tests.find_ref import ref_find_runs, ref_match

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _positions(starts, ends):
    return np.concatenate([np.arange(s, e) for s, e in zip(starts, ends)] + [np.zeros(0, np.int64)]).astype(np.int64)


def test_reference_equals_the_literal_expression():
    """scripts/query_index.py's "custom" branch on rows queried at step 1: the positions of the reference's runs are its
    np.flatnonzero, for 4 columns of 9 and of 33 genomes"""
    for n in (9, 33):
        rows = rc.dense(5000, n, 7 + n)
        kmers = rc.unpack(rows, n)
        want = np.flatnonzero((kmers[:, 0] == 1) & (kmers[:, 1] == 0) & (kmers[:, 2] == 1) & (kmers[:, 3] == 0))
        s, e, matched = ref_find_runs(rows, n, 0, len(rows), 1, [0, 2], [1, 3], 2, 0)
        assert len(want) > 100 and matched == len(want)
        assert np.array_equal(_positions(s, e), want)
        assert (s[1:] > e[:-1]).all()  # maximal: a non-matching row between any two runs
        # a window: the same positions cut to it
        s, e, matched = ref_find_runs(rows, n, 1000, 3000, 1, [0, 2], [1, 3], 2, 0)
        assert np.array_equal(_positions(s, e), want[(want >= 1000) & (want < 3000)])


def _col0(pattern):
    """rows of 3 genomes whose column 0 follows the string of 0 / 1 (column 1 is set everywhere, column 2 nowhere)"""
    bits = np.zeros((len(pattern), 3), np.uint8)
    bits[:, 0] = [int(c) for c in pattern]
    bits[:, 1] = 1
    return rc.pack(bits)


@pytest.mark.parametrize("pattern, stride, s, e, starts, ends", [
    ("110011100011", 1, 0, 12, [0, 4, 10], [2, 7, 12]),  # a run at row 0 and one at the last row
    ("111111111111", 1, 0, 12, [0], [12]),               # all rows
    ("000000000000", 1, 0, 12, [], []),                  # no row
    ("011111111110", 1, 3, 8, [3], [8]),                 # the window cuts a run on both sides
    ("011111111110", 1, 5, 5, [], []),                   # an empty window
    ("100100100100", 3, 0, 4, [0], [4]),                 # stride 3: rows 0, 3, 6, 9
    ("010010010011", 3, 0, 4, [], []),
    ("100000100100", 3, 0, 4, [0, 2], [1, 4]),
    ("100000100100", 3, 1, 3, [2], [3]),
])
def test_reference_on_a_dozen_rows(pattern, stride, s, e, starts, ends):
    gs, ge, matched = ref_find_runs(_col0(pattern), 3, s, e, stride, [0, 1], [2], 2, 0)
    assert gs.tolist() == starts and ge.tolist() == ends
    assert matched == sum(b - a for a, b in zip(starts, ends))


def test_reference_thresholds():
    rows = rc.ramp(40, 9)  # row i: its lowest i mod 10 bits
    popc = np.arange(40) % 10
    every = list(range(9))
    assert np.array_equal(ref_match(rows, 9, 1, every, [], 4, 0), popc >= 4)
    assert np.array_equal(ref_match(rows, 9, 1, [], every, 0, 4), popc <= 4)
    assert not ref_match(rows, 9, 1, [0, 1], [], 3, 0).any()   # min_have > |H|: legal, matches nothing
    assert ref_match(rows, 9, 1, [0, 1], [], 0, 0).all()       # min_have = 0 and no L: every row
    # pad bits do not count
    assert np.array_equal(ref_match(rc.with_pad_bits(rows, 9), 9, 1, [], every, 0, 4), popc <= 4)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 130])
def test_rule_words(n):
    names = [f"g{i}" for i in range(n)]
    have = sorted({0, n - 1, n // 2})
    lack = sorted(set(range(n)) - set(have))[:3]
    hw, lw, mh, ml = find.rule_words(names, [names[g] for g in have], [names[g] for g in lack])
    assert hw.dtype == np.uint32 and lw.dtype == np.uint32 and len(hw) == len(lw) == (n + 31) // 32
    assert np.array_equal(hw, rc.words_of(n, have)) and np.array_equal(lw, rc.words_of(n, lack))
    assert (mh, ml) == (len(have), 0)
    # column numbers, given thresholds, an empty lack set
    hw2, lw2, mh, ml = find.rule_words(names, have, (), min_have=0, max_lack=5)
    assert np.array_equal(hw2, hw) and not lw2.any() and (mh, ml) == (0, 5)
    assert find.rule_words(names, have, [], min_have=n + 7)[2] == n + 7  # cannot be met: legal


def test_rule_words_errors():
    names = ["a", "b", "c"]
    with pytest.raises(ValueError, match="'zz'"):
        find.rule_words(names, ["a", "zz"], [])
    with pytest.raises(ValueError, match="'zz'"):
        find.rule_words(names, ["a"], ["zz"])
    with pytest.raises(ValueError, match="out of range"):
        find.rule_words(names, [3], [])
    with pytest.raises(ValueError, match="both"):
        find.rule_words(names, ["a", "b"], ["b"])
    with pytest.raises(ValueError, match="both"):
        find.rule_words(names, ["a"], [0])
    with pytest.raises(ValueError, match="negative"):
        find.rule_words(names, ["a"], [], min_have=-1)
    with pytest.raises(ValueError, match="negative"):
        find.rule_words(names, ["a"], [], max_lack=-1)


def test_merge_runs():
    s, e = np.array([0, 5, 9, 20, 23]), np.array([2, 7, 10, 21, 30])  # gaps: 3, 2, 10, 2
    assert [x.tolist() for x in find.merge_runs(s, e)] == [s.tolist(), e.tolist(), [2, 2, 1, 1, 7]]
    # a gap of exactly max_gap merges, one of max_gap + 1 does not
    assert [x.tolist() for x in find.merge_runs(s, e, max_gap=2)] == [[0, 5, 20], [2, 10, 30], [2, 3, 8]]
    assert [x.tolist() for x in find.merge_runs(s, e, max_gap=3)] == [[0, 20], [10, 30], [5, 8]]
    assert [x.tolist() for x in find.merge_runs(s, e, max_gap=10)] == [[0], [30], [13]]
    # min_len is applied AFTER merging: [5, 10) is 5 rows long though its runs are 2 and 1
    assert [x.tolist() for x in find.merge_runs(s, e, min_len=5, max_gap=2)] == [[5, 20], [10, 30], [3, 8]]
    assert [x.tolist() for x in find.merge_runs(s, e, min_len=5)] == [[23], [30], [7]]
    assert [x.tolist() for x in find.merge_runs(s, e, min_len=100, max_gap=10)] == [[], [], []]
    # empty input
    for out in find.merge_runs([], [], 3, 4):
        assert out.dtype == np.int64 and len(out) == 0
    with pytest.raises(ValueError):
        find.merge_runs(s, e, min_len=0)
    with pytest.raises(ValueError):
        find.merge_runs(s, e, max_gap=-1)


def test_merge_runs_against_a_loop():
    rng = np.random.default_rng(3)
    m = rng.random(3000) < 0.6
    d = np.diff(np.concatenate([[0], m.astype(np.int8), [0]]))
    s, e = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    for min_len, max_gap in [(1, 0), (1, 1), (4, 0), (6, 2), (30, 3)]:
        want = []
        for a, b in zip(s, e):
            if want and a - want[-1][1] <= max_gap:
                want[-1][1] = b
            else:
                want.append([a, b])
        want = [(a, b, int(m[a:b].sum())) for a, b in want if b - a >= min_len]
        got = find.merge_runs(s, e, min_len, max_gap)
        assert list(zip(*(x.tolist() for x in got))) == want, (min_len, max_gap)


def test_join_pieces():
    z = np.zeros(0, np.int64)
    # a run across a boundary: piece 0 ends inside a run, piece 1 begins inside it
    s, e = find.join_pieces([(0, 10, [2, 7], [4, 10]), (10, 10, [0, 5], [3, 6])])
    assert s.tolist() == [2, 7, 15] and e.tolist() == [4, 13, 16]
    # a run ending exactly at the boundary with none beginning there
    s, e = find.join_pieces([(0, 10, [7], [10]), (10, 10, [1], [3])])
    assert s.tolist() == [7, 11] and e.tolist() == [10, 13]
    # ... and one beginning at the boundary with none ending there
    s, e = find.join_pieces([(0, 10, [7], [9]), (10, 10, [0], [3])])
    assert s.tolist() == [7, 10] and e.tolist() == [9, 13]
    # three pieces spanned by one run
    s, e = find.join_pieces([(0, 4, [1], [4]), (4, 3, [0], [3]), (7, 5, [0], [2])])
    assert s.tolist() == [1] and e.tolist() == [9]
    # pieces without runs, no piece at all
    s, e = find.join_pieces([(0, 4, z, z), (4, 4, [1], [2]), (8, 4, z, z)])
    assert s.tolist() == [5] and e.tolist() == [6] and s.dtype == np.int64
    s, e = find.join_pieces([])
    assert len(s) == 0 and len(e) == 0


def test_join_pieces_against_the_uncut_vector():
    rng = np.random.default_rng(5)
    m = rng.random(1000) < 0.7

    def runs(v):
        d = np.diff(np.concatenate([[0], v.astype(np.int8), [0]]))
        return np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    for per in (1, 2, 7, 100, 999, 1000, 5000):
        pieces = [(p0, len(m[p0:p0 + per]), *runs(m[p0:p0 + per])) for p0 in range(0, len(m), per)]
        s, e = find.join_pieces(pieces)
        assert np.array_equal(s, runs(m)[0]) and np.array_equal(e, runs(m)[1]), per


def test_chunk_constant_is_the_kernels():
    from panagram_amd import engine
    txt = open(os.path.join(ROOT, "panagram_amd", "csrc", "pg_kernels.h")).read()
    assert int(re.search(r"constexpr uint32_t FIND_CHUNK = (\d+);", txt).group(1)) == engine.FIND_CHUNK
    assert engine.FIND_CHUNK % 256 == 0 and engine.FIND_FIRST_CAP > 0
