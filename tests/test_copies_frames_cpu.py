"""CPU: panagram_amd/copies.py — the frames and the track lines of ``Index.copies`` on hand-written histograms, and the argument
rule of the ``copies`` subcommand."""
import numpy as np
import pytest

from panagram_amd import copies as cp

K = 21


def hist_of(**bins):
    h = np.zeros(cp.BINS, np.uint64)
    for c, n in bins.items():
        h[int(c[1:])] = n
    return h


def test_lower_median_at_even_and_odd_counts():
    # depths 1 1 2 2: the two middle values are 1 and 2, the lower one counts
    assert cp.lower_median(hist_of(b1=2, b2=2)) == 1
    # depths 1 2 2: the middle value is 2
    assert cp.lower_median(hist_of(b1=1, b2=2)) == 2
    # depths 0 0 0 5 5 5 5
    assert cp.lower_median(hist_of(b0=3, b5=4)) == 5
    assert cp.lower_median(hist_of(b0=4, b5=4)) == 0
    assert cp.lower_median(hist_of(b7=1)) == 7
    assert cp.lower_median(np.zeros(cp.BINS)) == 0
    both = cp.lower_median(np.stack([hist_of(b1=2, b2=2), hist_of(b1=1, b2=2)]))
    assert both.tolist() == [1, 2]


def frames_of(names, lens, genomes, hists):
    hist = np.array(hists, np.uint64).reshape(len(names), len(genomes), cp.BINS)
    valid = hist[:, 0].sum(axis=1) if len(genomes) else np.zeros(len(names), np.uint64)
    return cp.frames(names, lens, K, genomes, hist, valid)


def test_frames_columns_and_values():
    names, lens, genomes = ["t1", "t2"], [120, 30], ["A", "B"]
    hists = [[hist_of(b1=60, b2=40), hist_of(b0=70, b3=30)],
             [hist_of(b63=6, b1=4), hist_of(b0=10)]]
    long, matrix, summary = frames_of(names, lens, genomes, hists)
    assert list(long.columns) == cp.LONG_COLUMNS
    assert long["target"].tolist() == ["t1", "t1", "t2", "t2"] and long["genome"].tolist() == ["A", "B", "A", "B"]
    assert long["kmers"].tolist() == [100, 100, 10, 10] and long["valid"].tolist() == [100, 100, 10, 10]
    assert long["present"].tolist() == [100, 30, 10, 0]
    assert long["frac"].tolist() == [1.0, 0.3, 1.0, 0.0]
    assert long["copies"].tolist() == [1, 0, 63, 0]
    assert long["copies_nz"].tolist() == [1, 3, 63, 0]
    assert long["mean"].tolist() == [1.4, 0.9, (63 * 6 + 4) / 10, 0.0]
    assert long["mean_is_lower_bound"].tolist() == [False, False, True, False]
    assert long["max_bin"].tolist() == [2, 3, 63, 0]
    assert matrix.index.tolist() == names and matrix.columns.tolist() == genomes
    assert matrix.to_numpy().tolist() == [[1, 0], [63, 0]]
    assert list(summary.columns) == cp.SUMMARY_COLUMNS
    assert summary.to_numpy().tolist() == [["A", 2, 0, 1, 0, 0, 1], ["B", 2, 2, 0, 0, 0, 0]]


def test_the_last_bin_prints_open():
    long, matrix, _ = frames_of(["t"], [83], ["A"], [[hist_of(b63=63)]])
    text = cp.long_text(long)
    assert text["copies"].tolist() == ["63+"] and text["copies_nz"].tolist() == ["63+"] and text["max_bin"].tolist() == ["63+"]
    assert text["mean"].tolist() == [">=63.000"]
    assert "mean_is_lower_bound" not in text.columns
    assert cp.matrix_text(matrix).to_numpy().tolist() == [["63+"]]
    assert cp.copies_text(62) == "62" and cp.copies_text(63) == "63+"


def test_copies_nz_skips_the_absent_positions():
    # 70 positions absent, the others at depth 2 2 2 4: the median is 0, over the present ones the lower median is 2
    long, _, _ = frames_of(["t"], [93], ["A"], [[hist_of(b0=70, b2=2, b4=1)]])
    assert long["copies"].tolist() == [0] and long["copies_nz"].tolist() == [2]
    long, _, _ = frames_of(["t"], [93], ["A"], [[hist_of(b0=69, b2=2, b4=2)]])
    assert long["copies_nz"].tolist() == [2]
    long, _, _ = frames_of(["t"], [93], ["A"], [[hist_of(b0=68, b2=2, b4=3)]])
    assert long["copies_nz"].tolist() == [4]


def test_a_target_without_a_valid_position_stays():
    names, lens, genomes = ["short", "allN", "ok"], [5, 50, 40], ["A", "B"]
    z = np.zeros(cp.BINS, np.uint64)
    long, matrix, summary = frames_of(names, lens, genomes, [[z, z], [z, z], [hist_of(b2=20), hist_of(b1=20)]])
    assert long["target"].tolist() == ["short", "short", "allN", "allN", "ok", "ok"]
    assert long["kmers"].tolist() == [0, 0, 30, 30, 20, 20] and long["valid"].tolist() == [0, 0, 0, 0, 20, 20]
    first = long.iloc[:4]
    for c in ("present", "frac", "copies", "copies_nz", "mean", "max_bin"):
        assert (first[c] == 0).all()
    assert matrix.to_numpy().tolist() == [[0, 0], [0, 0], [2, 1]]
    assert summary.to_numpy().tolist() == [["A", 3, 2, 0, 1, 0, 0], ["B", 3, 2, 1, 0, 0, 0]]


def test_duplicate_names_and_order_are_kept():
    long, matrix, _ = frames_of(["x", "y", "x"], [30, 30, 30], ["B", "A"], [[hist_of(b1=10), hist_of(b2=10)], [hist_of(b3=10), hist_of(b4=10)],
                                                                          [hist_of(b5=10), hist_of(b6=10)]])
    assert matrix.index.tolist() == ["x", "y", "x"] and matrix.columns.tolist() == ["B", "A"]
    assert matrix.to_numpy().tolist() == [[1, 2], [3, 4], [5, 6]]
    assert long["copies"].tolist() == [1, 2, 3, 4, 5, 6]


def test_summary_classes():
    names = [f"t{i}" for i in range(7)]
    hists = [[hist_of(**{f"b{c}": 10})] for c in (0, 1, 2, 3, 4, 9, 63)]
    _, _, summary = frames_of(names, [30] * 7, ["A"], hists)
    assert summary.to_numpy().tolist() == [["A", 7, 1, 1, 1, 1, 3]]


def test_no_target_and_a_histogram_that_does_not_add_up():
    long, matrix, summary = cp.frames([], [], K, ["A"], np.zeros((0, 1, cp.BINS)), np.zeros(0))
    assert len(long) == 0 and matrix.shape == (0, 1) and summary.to_numpy().tolist() == [["A", 0, 0, 0, 0, 0, 0]]
    with pytest.raises(ValueError):
        cp.frames(["t"], [30], K, ["A"], hist_of(b1=9).reshape(1, 1, -1), [10])


def test_track_lines():
    # two targets of 5 and 3 positions (a third is shorter than k), two genomes
    lens = [K + 4, K - 1, K + 2]
    inv, top = cp.DEPTH_INVALID, cp.DEPTH_MAX
    depths = np.array([[1, 1, 2, 2, 2, 0, inv, inv],
                       [top, top, top, top, top, 7, 7, 7]], np.uint16)
    lines = list(cp.track_lines(["a", "b", "c"], lens, K, ["G", "H"], depths))
    assert lines == ["a\tG\t0\t2\t1", "a\tG\t2\t5\t2", f"a\tH\t0\t5\t{top}+", "c\tG\t0\t1\t0", "c\tG\t1\t3\t.", "c\tH\t0\t3\t7"]
    assert cp.TRACK_HEADER.split("\t") == ["target", "genome", "start", "end", "depth"]


def test_planes_for():
    assert cp.planes_for(1 << 30, 1 << 20, 100) == 100
    assert cp.planes_for(1 << 30, 1 << 24, 100) == ((1 << 29) - (8 << 24)) // (4 << 24)
    assert cp.planes_for(1 << 20, 1 << 24, 100) == 1  # (no room: one plane, and the table's creation says so)
    assert cp.planes_for(1 << 30, 1 << 20, 100, track_kmers=1 << 28) == 1


def test_table_slots():
    """the power of two at or above twice the capacity, as pg_copytable_create and pg_postable_create size their tables"""
    assert [cp.table_slots(c) for c in (1, 2, 3, 1 << 30)] == [2, 4, 8, 1 << 31]


@pytest.mark.parametrize("argv", [["copies", "idx"], ["copies", "idx", "t.fa", "--genes", "G"]])
def test_cli_wants_exactly_one_of_targets_and_genes(argv, capsys):
    from panagram_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert e.value.code == 2
    assert "exactly one of targets.fa and --genes" in capsys.readouterr().err


def test_cli_checks_before_it_opens_anything(tmp_path, capsys):
    from panagram_amd.__main__ import main
    for argv, word in ((["copies", str(tmp_path / "none"), "t.fa"], "not an index directory"),
                       (["copies", str(tmp_path), str(tmp_path / "t.fa")], "no target file"),
                       (["copies", str(tmp_path), "--genes", "G", "-k", "33"], "k=33")):
        with pytest.raises(SystemExit) as e:
            main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err
