"""CPU: the numpy model of synteny (tests/synteny_ref.py) on hand-built cases whose segments follow by construction, and the host
functions of panagram_amd/synteny.py.  The GPU tests hold the kernels to the model; this file holds the model to the definitions."""
import numpy as np
import pytest

from panagram_amd import synteny
from tests import synteny_ref as sr

K = sr.PLANTED_K  # odd: no k-mer is its own reverse complement
NO = sr.NO_MATE


def _random_unique(n, seed, k=K):
    """random codes whose k-mers are all distinct, both strands counted (the premise of every case below)"""
    codes = sr.random_codes(n, seed)
    keys, _, _, _ = sr.side_kmers([sr.ascii_of(codes)], k)
    assert len(np.unique(keys)) == n - k + 1
    return codes


def _planted_pair():
    x, y = sr.planted_contigs()
    keys, _, _, _ = sr.side_kmers([sr.ascii_of(x), sr.ascii_of(y)], K)
    assert len(np.unique(keys)) == len(keys)
    return x, y


def _runs(a, b, k=K):
    return sr.segments([sr.ascii_of(x) for x in a], [sr.ascii_of(x) for x in b], k)


def test_identity_gives_one_plus_run_per_contig():
    a = [_random_unique(700, 1), sr.random_codes(9, 2), _random_unique(400, 3)]  # (the middle contig is shorter than k)
    runs, mated = _runs(a, a)
    assert runs.tolist() == [[0, 0, 700 - K + 1, 0], [2, 0, 400 - K + 1, (700 + 9) << 1]]
    assert mated == 700 - K + 1 + 400 - K + 1


def test_reverse_complement_gives_one_minus_run_with_descending_positions():
    a = _random_unique(900, 4)
    m, nk = sr.mates([sr.ascii_of(a)], [sr.ascii_of(sr.revcomp(a))], K)
    n = 900 - K + 1
    assert nk == [n]
    assert m.tolist() == [((n - 1 - i) << 1) | 1 for i in range(n)]
    assert sr.runs(m, nk).tolist() == [[0, 0, n, ((n - 1) << 1) | 1]]


def test_palindromes_have_rc_zero_on_both_strands():
    # even k: ACGT is its own reverse complement, the forward value equals the other strand's, so rc = 0 wherever it stands
    a, b = b"GGACGTCC", b"TTACGTAA"
    m, nk = sr.mates([a], [b], 4)
    assert nk == [5] and m.tolist() == [NO, NO, (2 << 1) | 0, NO, NO]
    # and a k-mer against its reverse complement elsewhere in the SAME genome: two occurrences, no mate
    m, _ = sr.mates([b"AACCGTTTTGGAC"], [b"AACC"], 4)  # AACC at 0 (GGTT nowhere) -> mate; with GGTT added, none
    assert m[0] == 0
    m, _ = sr.mates([b"AACCGGGTTGGAC"], [b"AACC"], 4)  # GGTT at 5 is AACC's reverse complement
    assert m[0] == NO


def test_inverted_block_gives_plus_minus_plus_with_unmated_flanks():
    a = _random_unique(1200, 5)
    lo, hi = 400, 700
    a[lo] = a[hi - 1] = 0  # the base just inside either breakpoint changes under the inversion (A <-> T): every spanning k-mer differs
    keys, _, _, _ = sr.side_kmers([sr.ascii_of(a)], K)
    assert len(np.unique(keys)) == 1200 - K + 1
    b = sr.plant_inversion(a, lo, hi)
    runs, mated = _runs([a], [b])
    nk = 1200 - K + 1
    assert runs.tolist() == [[0, 0, lo - K + 1, 0], [0, lo, hi - K + 1, ((hi - K) << 1) | 1], [0, hi, nk, hi << 1]]
    assert mated == nk - 2 * (K - 1)


def test_duplicated_block_in_b_removes_its_kmers():
    a = _random_unique(1000, 6)
    lo, hi = 300, 500
    a[lo - 1], a[hi - 1] = 0, 1  # the second copy is not preceded by what precedes the first ...
    a[lo], a[hi] = 2, 3          # ... and the first is not followed by what follows the second
    keys, _, _, _ = sr.side_kmers([sr.ascii_of(a)], K)
    assert len(np.unique(keys)) == 1000 - K + 1
    b = sr.plant_tandem_duplication(a, lo, hi)
    runs, _ = _runs([a], [b])
    # k-mers inside the block occur twice in B; those that leave it at its end are found behind the second copy
    assert runs.tolist() == [[0, 0, lo, 0], [0, hi - K + 1, 1000 - K + 1, (hi - K + 1 + hi - lo) << 1]]


def test_snp_clears_k_positions_and_splits_the_run():
    a = _random_unique(800, 7)
    b = sr.plant_snps(a, [350])
    runs, mated = _runs([a], [b])
    assert runs.tolist() == [[0, 0, 350 - K + 1, 0], [0, 351, 800 - K + 1, 351 << 1]]
    assert mated == 800 - K + 1 - K


def test_two_contigs_of_a_adjacent_in_b_give_two_runs():
    s = _random_unique(900, 8)
    cut = 500
    a = [s[:cut + K - 1], s[cut:]]  # k-mers 0 .. cut - 1 and cut .. of S: the mates array has no break at the contig edge
    m, nk = sr.mates([sr.ascii_of(x) for x in a], [sr.ascii_of(s)], K)
    assert nk == [cut, 900 - K + 1 - cut] and m.tolist() == [i << 1 for i in range(900 - K + 1)]
    assert sr.runs(m, nk).tolist() == [[0, 0, cut, 0], [1, 0, 900 - K + 1 - cut, cut << 1]]


def test_translocation_to_another_contig():
    x, y = _planted_pair()
    b = sr.plant_translocation([x, y], 0, 200, 500, 1, 300)
    runs, _ = _runs([x, y], b)
    lb0 = 600
    assert runs.tolist() == [[0, 0, 200 - K + 1, 0], [0, 200, 500 - K + 1, (lb0 + 300) << 1], [0, 500, 900 - K + 1, 200 << 1],
                             [1, 0, 300 - K + 1, lb0 << 1], [1, 300, 700 - K + 1, (lb0 + 600) << 1]]
    rows = sr.segment_rows(runs, K, ["x", "y"], [600, 1000], ["bx", "by"])
    assert rows[1] == ("x", 200, 500, "by", 300, 600, "+", 300 - K + 1)
    assert rows[2] == ("x", 500, 900, "bx", 200, 600, "+", 400 - K + 1)


def test_runs_break_on_steps_and_strand_flips():
    # + strand: steps of +2 in the word continue; +4 (posB + 2), -2 (posB - 1) and a strand flip break
    m = np.array([10, 12, 16, 14, 15, 13, 11, NO, 21, 23, 20], np.uint32)
    assert sr.runs(m, [11]).tolist() == [[0, 0, 2, 10], [0, 2, 3, 16], [0, 3, 4, 14], [0, 4, 7, 15], [0, 8, 9, 21], [0, 9, 10, 23],
                                         [0, 10, 11, 20]]
    # contigs of 0 and 1 positions; a run to a contig's last position; the word 0xFFFFFFFE is a mate like any other
    m = np.array([NO, 4, 6, 7, NO - 1], np.uint32)
    assert sr.runs(m, [0, 3, 1, 0, 1]).tolist() == [[1, 1, 3, 4], [2, 0, 1, 7], [4, 0, 1, NO - 1]]


# ---------------------------------------------------------------------------
# panagram_amd/synteny.py
# ---------------------------------------------------------------------------
def test_segment_frame_base_ranges_on_both_strands():
    k = 5
    lens_b = [100, 0, 50]
    # a + run of 10 k-mers at posB 20 of the first contig; a - run of 4 k-mers whose first k-mer is the LAST of the third contig
    # (global 100 + 45): B's range ends at posB + k = the contig's end
    f = synteny.segment_frame([0, 1], [7, 0], [17, 4], [20 << 1, ((100 + 45) << 1) | 1], k, ["a1", "a2"], lens_b, ["b1", "b2", "b3"])
    assert list(f.columns) == synteny.COLUMNS
    assert f.values.tolist() == [["a1", 7, 21, "b1", 20, 34, "+", 10], ["a2", 0, 8, "b3", 42, 50, "-", 4]]
    assert ((f["endA"] - f["startA"]) == f["kmers"] + k - 1).all() and ((f["endB"] - f["startB"]) == f["kmers"] + k - 1).all()
    # the model's plain loop says the same
    assert [tuple(r) for r in f.values.tolist()] == sr.segment_rows([[0, 7, 17, 40], [1, 0, 4, 291]], k, ["a1", "a2"], lens_b, ["b1", "b2", "b3"])
    # a run that would cross a contig edge of B, or leave B, is refused
    with pytest.raises(ValueError):
        synteny.segment_frame([0], [0], [10], [95 << 1], k, ["a1"], lens_b, ["b1", "b2", "b3"])
    with pytest.raises(ValueError):
        synteny.segment_frame([0], [0], [3], [(1 << 1) | 1], k, ["a1"], lens_b, ["b1", "b2", "b3"])
    # no run at all: an empty frame with the columns
    e = synteny.segment_frame([], [], [], [], k, ["a1"], lens_b, ["b1", "b2", "b3"])
    assert list(e.columns) == synteny.COLUMNS and len(e) == 0


def test_min_len_filter_and_summary_sums():
    x, y = _planted_pair()
    b = sr.planted_rearranged(x, y)
    a = [sr.ascii_of(x), sr.ascii_of(y)]
    bb = [sr.ascii_of(c) for c in b]
    runs, mated = sr.segments(a, bb, K)
    lens_b = [len(c) for c in bb]
    f = synteny.segment_frame(runs[:, 0], runs[:, 1], runs[:, 2], runs[:, 3], K, ["x", "y"], lens_b, ["bx", "by"])
    assert [tuple(r) for r in f.values.tolist()] == sr.segment_rows(runs, K, ["x", "y"], lens_b, ["bx", "by"])
    assert int(f["kmers"].sum()) == mated
    s = synteny.summary_frame(f)
    assert list(s.columns) == synteny.SUMMARY_COLUMNS
    assert s.iloc[-1].tolist() == ["*", "*", "*", len(f), mated]
    pairs = s[(s["chrA"] != "*") & (s["chrB"] != "*")]
    assert int(pairs["kmers"].sum()) == mated and int(pairs["segments"].sum()) == len(f)
    for side, other in (("chrA", "chrB"), ("chrB", "chrA")):
        per = s[(s[side] != "*") & (s[other] == "*")]
        assert int(per["kmers"].sum()) == mated and set(per[side]) == set(f[side])
        for name, n in zip(per[side], per["kmers"]):
            assert n == int(f.loc[f[side] == name, "kmers"].sum())
    assert ("y", "by", "-") in set(zip(pairs["chrA"], pairs["chrB"], pairs["strand"]))
    # min_len: the inverted block of 40 bases holds 26 k-mers
    short = synteny.segment_frame(runs[:, 0], runs[:, 1], runs[:, 2], runs[:, 3], K, ["x", "y"], lens_b, ["bx", "by"], min_len=27)
    assert short.values.tolist() == f[f["kmers"] >= 27].values.tolist() and len(short) == len(f) - 1
    assert "-" not in set(short["strand"])
    with pytest.raises(ValueError):
        synteny.segment_frame([], [], [], [], K, ["x"], [1], ["b"], min_len=0)
    assert synteny.summary_frame(f.iloc[:0]).values.tolist() == [["*", "*", "*", 0, 0]]


def test_chromosome_maps():
    offs = synteny.contig_offsets([10, 0, 0, 5, 7])
    assert offs.tolist() == [0, 10, 10, 10, 15, 22]
    c, o = synteny.locate([0, 9, 10, 14, 15, 21], offs)
    assert c.tolist() == [0, 0, 3, 3, 4, 4] and o.tolist() == [0, 9, 0, 4, 0, 6]
    assert synteny.pick_contigs(["c1", "c2", "c3"], None) == [0, 1, 2]
    assert synteny.pick_contigs(["c1", "c2", "c3"], ["c3", "c1"]) == [0, 2]  # (the sequence set's order)
    with pytest.raises(ValueError, match="nobody"):
        synteny.pick_contigs(["c1"], ["nobody"])
    with pytest.raises(ValueError):
        synteny.pick_contigs(["c1"], ["c1", "c1"])
    f = synteny.segment_frame([0, 0, 1], [0, 50, 0], [30, 60, 20], [0, (200 + 5) << 1, ((100 + 60) << 1) | 1], 5, ["a1", "a2"], [100, 100, 100],
                              ["b1", "b2", "b3"])
    m = synteny.chromosome_map(f)
    assert m.values.tolist() == [["a1", "b1", 30, 40, 0.0], ["a2", "b2", 20, 20, 1.0]]


def test_totals_and_the_summary_file(tmp_path):
    import pandas as pd
    x, y = _planted_pair()
    a = [sr.ascii_of(x), sr.ascii_of(y)]
    b = [sr.ascii_of(c) for c in sr.planted_rearranged(x, y)]
    runs, mated = sr.segments(a, b, K)
    # a genome against itself: the positions whose k-mer is unique in it — what the totals' `unique` column is computed from
    for side in (a, b):
        m, _ = sr.mates(side, side, K)
        assert int((m != NO).sum()) == len(sr.unique_of(sr.side_kmers(side, K)[0])[0])
    ua, ub = (len(sr.unique_of(sr.side_kmers(s, K)[0])[0]) for s in (a, b))
    t = synteny.totals_frame("ga", "gb", ua, ub, mated)
    assert list(t.columns) == synteny.TOTALS_COLUMNS and t.values.tolist() == [["A", "ga", ua, mated], ["B", "gb", ub, mated]]
    assert mated <= min(ua, ub)
    f = synteny.segment_frame(runs[:, 0], runs[:, 1], runs[:, 2], runs[:, 3], K, ["x", "y"], [len(c) for c in b], ["bx", "by"])
    path = tmp_path / "summary.tsv"
    synteny.write_summary(path, synteny.summary_frame(f), t)
    lines = path.read_text().splitlines()
    assert lines[:3] == ["# side\tgenome\tunique\tmated", f"# A\tga\t{ua}\t{mated}", f"# B\tgb\t{ub}\t{mated}"]
    back = pd.read_csv(path, sep="\t", comment="#")
    assert back.values.tolist() == synteny.summary_frame(f).values.tolist()
