"""CPU: the numpy model of screen (tests/screen_ref.py) on identities that follow by construction, the crafted sample's promises,
and the host side — screen.frames' ranking, ties, identity, zero denominators and genome selection, the min_count default rule,
the writers, and the subcommand's arguments."""
import io
import re

import numpy as np
import pytest

from oracle import pyoracle as po
from panagram_amd import screen as scr
from tests import kmerstats_ref as KR
from tests import screen_ref as SR


def test_constants_agree_with_the_kernels_header():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "panagram_amd", "csrc", "pg_kernels.h")).read()
    m = re.search(r"SCREEN_BINS = (\d+), SCREEN_DEPTH_MAX = (\d+)", txt)
    assert m and int(m.group(1)) == SR.BINS and int(m.group(2)) == SR.DEPTH_MAX == scr.DEPTH_MAX
    src = open(os.path.join(root, "panagram_amd", "engine.py")).read()  # (not imported: that would load the library)
    assert re.search(r"^SCREEN_BINS = 64\b", src, re.M) and re.search(r"^SCREEN_DEPTH_MAX = 255\b", src, re.M)


@pytest.mark.parametrize("k", [15, 21, 31, 32])
@pytest.mark.parametrize("min_count", [1, 2, 3])
def test_the_crafted_sample_keeps_its_promises(k, min_count):
    rng = np.random.default_rng(k)
    keys = SR.table_keys(rng, 3000, k)
    assert len(keys) == 3000 == len(np.unique(keys))
    sets, p = SR.crafted_sample(keys, k, min_count, np.random.default_rng(100 + k))
    windows, hits, d = SR.depths(keys, sets, k)
    depth = dict(zip(keys.tolist(), d.tolist()))
    assert depth[p["below"]] == min_count - 1 and depth[p["at"]] == min_count
    # the homopolymer: more windows than a byte holds, all on one key
    assert SR.HOMOPOLYMER_RUN - k + 1 > SR.DEPTH_MAX and depth[p["homo"]] == SR.DEPTH_MAX
    if k == 21:
        assert SR.HOMOPOLYMER_RUN - k + 1 == 280
    # the satellite: three keys share its windows
    assert len(p["sat"]) == 3 and sum(depth[s] for s in p["sat"]) == SR.SATELLITE_BASES - k + 1
    assert min(depth[s] for s in p["sat"]) >= (SR.SATELLITE_BASES - k + 1) // 3
    # a key the table lacks, spelled on both strands: two windows that are no hit
    _, u, c = SR.sample_counts(sets, k)
    assert p["absent"] not in depth and c[np.searchsorted(u, np.uint64(p["absent"]))] == 2
    assert windows > hits > 0
    # the N-broken contig: of its k + 2 windows only the last exists; lower case counts; exactly k: one window; shorter: none
    assert depth[p["broken"]] == 1 and depth[p["lower"]] == 1 and depth[p["exact"]] == 1
    flat = [c for s in sets for c in s]
    assert p["short"] in flat and len(p["short"]) < k
    assert any(len(c) == k for c in flat) and any(b"N" in c and b"n" in c for c in flat) and any(c.islower() for c in flat)
    # the second set completes the depth of `at`: two calls make it
    assert SR.depths(keys, sets[:1], k)[2][keys.tolist().index(p["at"])] == min_count - 1
    # the body: depths 1, 2 and 3 all occur
    assert all((d == v).sum() > 10 for v in (0, 1, 2, 3))


def test_the_model_on_a_case_worked_by_hand():
    keys = np.array([3, 5, 9, 11], np.uint64)
    M = np.array([[1, 1, 1], [1, 0, 0], [0, 1, 0], [0, 1, 1]])
    got = SR.screen(keys, M, [2, 1, 0, 300 - 45], 2)
    assert got["distinct"].tolist() == [2, 3, 2] and got["seen"].tolist() == [1, 2, 2]
    assert got["private"].tolist() == [1, 1, 0] and got["private_seen"].tolist() == [0, 0, 0]
    assert got["occ"].tolist() == [0, 2, 1, 1] and got["seen_occ"].tolist() == [0, 0, 1, 1]
    assert got["depth_hist"][:3].tolist() == [1, 1, 1] and got["depth_hist"][63] == 1 and got["depth_hist"].sum() == 4
    assert got["core_depth_hist"][2] == 1 and got["core_depth_hist"].sum() == 1 and got["nkeys"] == 4
    one = SR.screen(keys, M, [2, 1, 0, 255], 1)
    assert one["seen"].tolist() == [2, 2, 2] and one["private_seen"].tolist() == [1, 0, 0]
    top = SR.screen(keys, M, [2, 1, 0, 255], 255)
    assert top["seen"].tolist() == [0, 1, 1]
    for bad in (0, 256, 1000):
        with pytest.raises(ValueError, match="min_count"):
            SR.screen(keys, M, [0, 0, 0, 0], bad)


def test_a_genomes_own_kmers_recover_it_whole():
    k, n = 21, 4
    genomes = [[po.codes_to_ascii(c) for c in g] for g in po.synth_genomes(n, [6000, 900], 0.03, 11)]
    keys, M = KR.from_groups(po.build_bitvec_dbs(genomes, k), n)
    for g in range(n):
        got, windows, hits = SR.screen_sets(keys, M, [genomes[g]], k, 1)
        assert got["seen"][g] == got["distinct"][g] > 0 and got["private_seen"][g] == got["private"][g] > 0
        assert got["seen_occ"][n] == got["occ"][n] > 0  # (the core is in every genome)
        assert windows == hits == sum(len(c) - k + 1 for c in genomes[g])
        others = [h for h in range(n) if h != g]
        assert (got["private_seen"][others] == 0).all() and (got["seen"][others] < got["distinct"][others]).all()
        assert got["depth_hist"].sum() == got["nkeys"] == len(keys)
    # every genome at once: everything is seen
    got, _, _ = SR.screen_sets(keys, M, genomes, k, 1)
    assert got["seen"].tolist() == got["distinct"].tolist() and got["seen_occ"].tolist() == got["occ"].tolist()
    assert got["core_depth_hist"][:n].sum() == 0  # (a core k-mer occurs in all n genomes)


def _counts(distinct, seen, private, pseen, occ=None, socc=None, core_hist=None, nkeys=0):
    n = len(distinct)
    z = np.zeros(n + 1, np.int64)
    return dict(distinct=np.array(distinct), seen=np.array(seen), private=np.array(private), private_seen=np.array(pseen),
                occ=z if occ is None else np.array(occ), seen_occ=z if socc is None else np.array(socc),
                depth_hist=np.zeros(64, np.int64), core_depth_hist=np.zeros(64, np.int64) if core_hist is None else np.array(core_hist),
                nkeys=nkeys)


def test_frames_ranking_ties_identity_zero_denominators_and_selection():
    names = ["a", "b", "c", "d", "e"]
    # a and c tie on containment (1/2), c has the higher private containment; d and e tie on both: index order; b has no k-mer
    counts = _counts([100, 0, 50, 10, 20], [50, 0, 25, 1, 2], [10, 0, 10, 0, 0], [1, 0, 5, 0, 0],
                     occ=[0, 20, 5, 0, 0, 40], socc=[0, 6, 1, 0, 0, 30], nkeys=65)
    main, occupancy, stats = scr.frames(counts, names, 21, 2, windows=1000, hits=750, reads=10, read_bases=1200)
    assert main.columns.tolist() == scr.MAIN_COLUMNS and main["genome"].tolist() == names
    assert main["rank"].tolist() == [2, 5, 1, 3, 4]
    assert main["containment"].tolist() == [0.5, 0.0, 0.5, 0.1, 0.1]
    assert main["private_containment"].tolist() == [0.1, 0.0, 0.5, 0.0, 0.0]  # (0 / 0 reads 0)
    assert np.allclose(main["identity"], np.array([0.5, 0.0, 0.5, 0.1, 0.1]) ** (1 / 21), rtol=0, atol=1e-15)
    assert occupancy.columns.tolist() == scr.OCCUPANCY_COLUMNS and occupancy["n"].tolist() == list(range(6))
    assert occupancy["kmers"].tolist() == [0, 20, 5, 0, 0, 40] and occupancy["seen"].tolist() == [0, 6, 1, 0, 0, 30]
    assert list(stats) == scr.STAT_NAMES
    assert (stats["reads"], stats["read_bases"], stats["windows"], stats["hits"]) == (10, 1200, 1000, 750)
    assert stats["hit_frac"] == 0.75 and stats["novel_frac"] == 0.25
    assert (stats["nkeys"], stats["keys_seen"], stats["core"], stats["core_seen"], stats["core_containment"]) == (65, 37, 40, 30, 0.75)
    assert stats["min_count"] == 2 and stats["depth_mode"] == 0
    # a selection keeps index order and the ranks among all
    sel, _, _ = scr.frames(counts, names, 21, 2, genomes=["e", "a"])
    assert sel["genome"].tolist() == ["a", "e"] and sel["rank"].tolist() == [2, 4]
    with pytest.raises(KeyError, match="nobody"):
        scr.frames(counts, names, 21, 2, genomes=["a", "nobody"])
    # nothing streamed, nothing in the table: zeros, no NaN
    empty = _counts([0, 0], [0, 0], [0, 0], [0, 0])
    main, _, stats = scr.frames(empty, ["x", "y"], 21, 1)
    assert main["rank"].tolist() == [1, 2] and not main.isna().any().any()
    assert stats["hit_frac"] == 0.0 and stats["novel_frac"] == 0.0 and stats["core_containment"] == 0.0


def test_depth_mode_is_taken_from_min_count_up():
    hist = np.zeros(64, np.int64)
    hist[1], hist[2], hist[12], hist[13] = 500, 90, 80, 80
    counts = _counts([1], [1], [0], [0], core_hist=hist)
    assert scr.frames(counts, ["a"], 21, 1)[2]["depth_mode"] == 1
    assert scr.frames(counts, ["a"], 21, 2)[2]["depth_mode"] == 2
    assert scr.frames(counts, ["a"], 21, 3)[2]["depth_mode"] == 12  # (the lowest depth on a tie)
    assert scr.frames(counts, ["a"], 21, 14)[2]["depth_mode"] == 0


def test_min_count_default_and_range():
    assert scr.default_min_count(True) == 2 and scr.default_min_count(False) == 1
    assert scr.check_min_count(1) == 1 and scr.check_min_count(255) == 255
    for bad in (0, -1, 256):
        with pytest.raises(ValueError, match="min_count"):
            scr.check_min_count(bad)
    from panagram_amd.index import is_fastq
    assert [is_fastq(p) for p in ("s.fq", "s.fastq.gz", "s.fq.gz", "s.fa", "s.fasta.gz")] == [True, True, True, False, False]


def test_the_writers(tmp_path):
    counts = _counts([4, 2], [3, 0], [1, 1], [1, 0], occ=[0, 2, 2], socc=[0, 1, 2], nkeys=4)
    main, occupancy, stats = scr.frames(counts, ["a", "b"], 21, 1, windows=8, hits=6, reads=2, read_bases=48)
    o = io.StringIO()
    scr.write_main(main, o)
    lines = o.getvalue().split("\n")
    assert lines[0].split("\t") == scr.MAIN_COLUMNS
    assert lines[1].split("\t") == ["a", "4", "3", "0.750000", f"{0.75 ** (1 / 21):.6f}", "1", "1", "1.000000", "1"]
    assert lines[2].split("\t")[:4] == ["b", "2", "0", "0.000000"] and lines[3] == ""
    scr.write_summary(stats, tmp_path / "s.tsv")
    got = (tmp_path / "s.tsv").read_text().split("\n")
    assert got[0] == "# reads\t2" and got[4] == "# hit_frac\t0.750000" and got[5] == "# novel_frac\t0.250000"
    assert [g.split("\t")[0][2:] for g in got[:-1]] == scr.STAT_NAMES
    scr.write_occupancy(occupancy, tmp_path / "o.tsv")
    assert (tmp_path / "o.tsv").read_text() == "n\tkmers\tseen\n0\t0\t0\n1\t2\t1\n2\t2\t2\n"


def test_subcommand_arguments(tmp_path, capsys):
    from panagram_amd.__main__ import main
    fq = tmp_path / "s.fq"
    fq.write_text("@r\nACGT\n+\nIIII\n")
    for argv, what in ((["screen"], "required"),
                       (["screen", str(tmp_path / "nowhere"), str(fq)], "not an index directory"),
                       (["screen", str(tmp_path), str(tmp_path / "no.fq")], "no sample file"),
                       (["screen", str(tmp_path), str(fq), "--min-count", "0"], "--min-count is 1 to 255"),
                       (["screen", str(tmp_path), str(fq), "--min-count", "256"], "--min-count is 1 to 255"),
                       (["screen", str(tmp_path), str(fq), "--batch-bytes", "0"], "--batch-bytes positive"),
                       (["screen", str(tmp_path), str(fq), "--min-count", "x"], "invalid int value")):
        with pytest.raises(SystemExit) as ei:
            main(argv)
        assert ei.value.code == 2
        assert what in capsys.readouterr().err, argv


def test_the_planted_sample_ranks_its_donors_under_the_model():
    """what tests/test_gpu_screen_e2e.py relies on, with the model alone: the donors B and C rank above A, and of A's private
    k-mers — which neither donor holds — the reads show at most 1 % at min_count 2 (a private k-mer of A is seen only when errors
    or the sample's own substitutions spell it twice)"""
    main, occupancy, stats = SR.e2e_model("reads", 2)
    rank = dict(zip(main["genome"], main["rank"]))
    assert rank["A"] == 3 and {rank["B"], rank["C"]} == {1, 2}
    row = main.set_index("genome").loc["A"]
    print("A: private", row["private"], "private_seen", row["private_seen"], "depth_mode", stats["depth_mode"], "novel", stats["novel_frac"])
    assert row["private"] > 1000 and 100 * row["private_seen"] <= row["private"], (row["private_seen"], row["private"])
    assert stats["depth_mode"] >= 4 and 0.0 < stats["novel_frac"] < 0.5  # (12-fold reads of 100 bases: deep enough, errors among them)
    assert occupancy["kmers"].sum() == stats["nkeys"] and stats["min_count"] == 2
    # B's own assembly at min_count 1 recovers B whole and no private k-mer of the others
    from tests import place_ref as pr
    main, _, stats = SR.e2e_model(pr.e2e_genomes()[0][1], 1)
    row = main.set_index("genome")
    assert row.loc["B", "containment"] == 1.0 and row.loc["B", "private_seen"] == row.loc["B", "private"] > 0
    assert row.loc["A", "private_seen"] == 0 and row.loc["C", "private_seen"] == 0 and stats["novel_frac"] == 0.0
