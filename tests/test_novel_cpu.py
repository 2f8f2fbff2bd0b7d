"""CPU: the numpy model of pg_novel.hip (tests/novel_ref.py) held to a brute-force dict walk and to what follows by construction; the
crafted sample held to its promises; panagram_amd/novel.py's frames, filters and writers; the `novel` subcommand's refusals."""
import io

import numpy as np
import pytest

from panagram_amd import novel as nov
from tests import novel_ref as NR
from tests import screen_ref as SR

KS = [6, 21, 31, 32]
MIN_COUNT = 2


@pytest.mark.parametrize("k", KS)
def test_model_equals_the_brute_force_walk(k):
    table, sets, R, _ = NR.crafted(k, MIN_COUNT)
    for upto in (1, 2):
        windows, hits, nk, d = NR.novel_counts(table, sets[:upto], k)
        bw, bh, bd = NR.brute(table, sets[:upto], k)
        assert (windows, hits) == (bw, bh)
        assert dict(zip(nk.tolist(), d.tolist())) == bd
        assert windows - hits == int(d.sum()) and not np.isin(nk, table).any()
    rc, ra, rb, lh, rh, windows, novel = NR.runs(table, R, k)
    assert list(zip(rc.tolist(), ra.tolist(), rb.tolist(), lh.tolist(), rh.tolist())) == NR.brute_runs(table, R, k)
    assert novel == int((rb - ra).sum()) and windows == NR.novel_counts(table, [R], k)[0]


@pytest.mark.parametrize("k", KS)
def test_the_crafted_sample_keeps_its_promises(k):
    table, sets, R, p = NR.crafted(k, MIN_COUNT)
    assert len(np.unique(table)) == len(table) and p["homo"] not in set(table.tolist())
    first = dict(zip(*(x.tolist() for x in NR.novel_counts(table, sets[:1], k)[2:])))
    windows, hits, nk, d = NR.novel_counts(table, sets, k)
    both = dict(zip(nk.tolist(), d.tolist()))
    # held keys never enter; every held key spelled is a hit
    assert np.isin(p["held"], table).all() and not set(p["held"].tolist()) & set(both) and hits >= 320
    assert set(int(x) for x in SR.special_keys(k)[1]) <= set(table.tolist())  # (the period-3 satellite ACG is held)
    # one key and one counter past what a byte holds; the satellites; the deep bin
    assert both[p["homo"]] == NR.HOMOPOLYMER_WINDOWS > 255
    assert len(p["sat3"]) == 3 and sum(both[x] for x in p["sat3"]) == NR.SAT3_BASES - k + 1
    assert len(p["sat11"]) == 11 > 8 and sum(both[x] for x in p["sat11"]) == NR.LONG_POSITIONS
    assert min(both[x] for x in p["sat11"]) >= 64 and NR.LONG_POSITIONS > 2 * NR.JOB + 300
    # the period-11 keys stand on both sides of either job edge
    long_c = sets[1][-1]
    for edge in (NR.JOB, 2 * NR.JOB):
        left = set(NR.cr.valid_keys([long_c[edge - 64:edge + k - 1]], k).tolist())
        right = set(NR.cr.valid_keys([long_c[edge:edge + 64 + k - 1]], k).tolist())
        assert left == right == set(p["sat11"])
    if k >= NR.EXACT_FROM_K:
        assert both[p["twice"]] == 2 and first[p["twice"]] == 1
        assert first.get(p["edge"], 0) == MIN_COUNT - 1 and both[p["edge"]] == MIN_COUNT
        assert both[p["broken"]] == 1 and both[p["lower"]] == 1 and both[p["exact"]] == 1
    res = NR.result(d, MIN_COUNT)
    assert res["depth_hist"][63] >= 12 and res["depth_hist"][1] > 0 and 0 < res["solid"] < res["nkeys"]
    # N and lower case, contigs of k - 1 and k bases
    flat = [c for s in sets for c in s]
    assert any(b"N" in c and b"n" in c for c in flat) and any(c.islower() for c in flat)
    assert {k - 1, k} <= {len(c) for c in flat}
    # the run contigs
    rc, ra, rb, lh, rh, _, _ = NR.runs(table, R, k)
    bases = NR.bases(ra, rb, lh, rh, k)
    by = {name: [(int(a), int(b), int(l), int(r), int(n)) for c, a, b, l, r, n in zip(rc, ra, rb, lh, rh, bases) if c == i]
          for name, i in p["runs"].items()}
    assert len(R[p["runs"]["short"]]) == k - 1 and by["short"] == [] and by["plain"] == []
    assert by["homo"] == [(0, 10, 0, 0, k + 9)]
    assert {(l, r) for runs in by.values() for _, _, l, r, _ in runs} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(a < NR.TILE < b for a, b, _, _, _ in by["tile"]) and any(a < NR.CHUNK < b for a, b, _, _, _ in by["chunk"])
    assert by["start_a"][0][0] == 0 and by["start_a"][0][1] >= 11 and by["start_a"][0][2] == 0
    n_end = len(R[p["runs"]["end_a"]]) - k + 1
    assert by["end_a"][-1][1] == n_end and by["end_a"][-1][0] <= n_end - 11 and by["end_a"][-1][3] == 0
    n_end = len(R[p["runs"]["end"]]) - k + 1
    assert len(by["cut"]) >= 2 and any(r == 0 for _, _, _, r, _ in by["cut"]) and any(l == 0 for _, _, l, _, _ in by["cut"])
    if k >= NR.EXACT_FROM_K:
        assert by["sub"] == [(400 - k + 1, 401, 1, 1, 1)]
        assert by["ins"] == [(500 - k + 1, 500 + NR.INSERTION, 1, 1, NR.INSERTION)]
        assert by["del"] == [(p["del_at"] - k + 1, p["del_at"], 1, 1, 0)]
        assert by["all"] == [(0, 333 - k + 1, 0, 0, 333)]
        assert by["start"] == [(0, 50, 0, 1, 50)] and by["end"] == [(600 - k + 1, n_end, 1, 0, 45)]
        assert [(l, r) for _, _, l, r, _ in by["cut"]] == [(1, 0), (0, 1)] and sum(n for *_, n in by["cut"]) == 60
        # what the run scan decides from a neighbour that is not the lane below: runs starting at a wave's, a tile's and a chunk's
        # first position, a run whose last position is a chunk's last, and a run closed at the contig's end — where the contig is
        # a whole number of tiles (edges) and where it is not (end_a)
        n_edges = len(R[p["runs"]["edges"]]) - k + 1
        assert n_edges == NR.EDGES_POSITIONS <= 2 * NR.CHUNK + 300 and n_edges % NR.TILE == 0 and n_end % NR.TILE != 0
        assert [r[:4] for r in by["edges"]] == [(NR.WAVE, NR.WAVE + k, 1, 1), (NR.TILE, NR.TILE + k, 1, 1), (NR.CHUNK - k, NR.CHUNK, 1, 1),
                                                (2 * NR.CHUNK, 2 * NR.CHUNK + k, 1, 1), (n_edges - k, n_edges, 1, 0)]


def test_bases_on_the_four_edge_pairs():
    k = 21
    # a run [a, b) of n = b - a novel positions: held on both sides the windows beside it cover k - 1 bases of either end
    for a, b in ((100, 121), (100, 158), (100, 120), (100, 101), (0, 313)):
        n = b - a
        want = {(1, 1): max(0, n - (k - 1)), (1, 0): n, (0, 1): n, (0, 0): n + k - 1}
        for (l, r), w in want.items():
            assert nov.run_bases([a], [b], [l], [r], k).tolist() == [w] == NR.bases([a], [b], [l], [r], k).tolist(), (a, b, l, r)
    # a substitution, an insertion of L, a deletion junction, a wholly novel contig of 333 bases
    assert nov.run_bases([380, 480, 480, 0], [401, 537, 500, 313], [1, 1, 1, 0], [1, 1, 1, 0], k).tolist() == [1, 37, 0, 333]


def _counts():
    hist = np.zeros(64, np.int64)
    hist[1], hist[2], hist[7], hist[8], hist[63] = 50, 4, 9, 9, 2
    return dict(nkeys=74, solid=24, solid_windows=4 * 2 + 9 * 7 + 9 * 8 + 300 + 70, depth_hist=hist)


def test_frames_filters_and_statistics():
    counts = _counts()
    regions = nov.regions_frame("s.fa", ["c1", "c2"], [0, 0, 1], [380, 480, 0], [401, 500, 313], [1, 1, 0], [1, 1, 0], 21)
    assert list(regions.columns) == nov.REGION_COLUMNS
    assert regions["end"].tolist() == [421, 520, 333] and regions["kmers"].tolist() == [21, 20, 313]
    assert regions["bases"].tolist() == [1, 0, 333] and regions["contig"].tolist() == ["c1", "c1", "c2"]
    assert (regions["end"] == regions["start"] + regions["kmers"] + 21 - 1).all()
    assert nov.filter_regions(regions, 0).equals(regions)
    kept = nov.filter_regions(regions, 1)
    assert kept["bases"].tolist() == [1, 333] and kept.index.tolist() == [0, 1]
    assert len(nov.filter_regions(regions, 334)) == 0
    with pytest.raises(ValueError, match="min_bases"):
        nov.filter_regions(regions, -1)
    st = nov.stats(counts, 2, windows=1000, hits=437, reads=3, read_bases=1060, regions=kept)
    assert list(st) == nov.STAT_NAMES
    assert st["novel_windows"] == 563 and st["novel_kmers"] == 74 and st["solid_kmers"] == 24 and st["solid_windows"] == 513
    assert st["error_windows"] == 50 and st["solid_frac"] == 24 / 74 and st["regions"] == 2 and st["region_bases"] == 334
    assert st["depth_mode"] == 7 and nov.stats(counts, 1)["depth_mode"] == 1 and nov.stats(counts, 9)["depth_mode"] == 63  # (the lowest on a tie)
    empty = nov.stats(dict(nkeys=0, solid=0, solid_windows=0, depth_hist=np.zeros(64, np.int64)), 1)
    assert empty["solid_frac"] == 0.0 and empty["depth_mode"] == 0 and empty["regions"] == 0
    sp = nov.spectrum_frame(counts["depth_hist"])
    assert list(sp.columns) == nov.SPECTRUM_COLUMNS and sp["depth"].tolist() == list(range(1, 64)) and sp["kmers"].sum() == 74
    keys = np.array([SR.canonical(b"ACGTTGCAAGT", 11), SR.canonical(b"AAAAAAAAAAC", 11)], np.uint64)
    km = nov.kmers_frame(keys, [5, 2], 11)
    assert list(km.columns) == nov.KMER_COLUMNS and km["kmer"].tolist() == sorted(SR.spell(int(x), 11).decode() for x in keys)
    assert km["depth"].tolist() == [2, 5] and nov.spell([int(keys[0])], 11) == [SR.spell(int(keys[0]), 11).decode()]
    assert nov.spell(np.array([(1 << 64) - 2], np.uint64), 32) == ["T" * 31 + "G"]
    assert len(nov.no_regions()) == 0 and list(nov.no_regions().columns) == nov.REGION_COLUMNS


def test_min_count_default_and_range():
    assert nov.default_min_count(True) == 2 and nov.default_min_count(False) == 1
    assert nov.check_min_count(1) == 1 and nov.check_min_count(300) == 300 and nov.check_min_count(2 ** 32 - 1) == 2 ** 32 - 1
    for bad in (0, -1, 2 ** 32):
        with pytest.raises(ValueError, match="min_count"):
            nov.check_min_count(bad)


def test_the_writers(tmp_path):
    counts = _counts()
    regions = nov.regions_frame("s.fa", ["c1"], [0], [380], [401], [1], [1], 21)
    st = nov.stats(counts, 2, windows=1000, hits=437, reads=3, read_bases=1060, regions=regions)
    o = io.StringIO()
    nov.write_stats(st, o)
    lines = o.getvalue().split("\n")
    assert [ln.split("\t")[0] for ln in lines[:-1]] == nov.STAT_NAMES and lines[-1] == ""
    assert lines[0] == "reads\t3" and lines[8] == f"solid_frac\t{24 / 74:.6f}" and lines[13] == "min_count\t2"
    nov.write_summary(st, tmp_path / "s.tsv")
    assert (tmp_path / "s.tsv").read_text() == o.getvalue()
    nov.write_regions(regions, tmp_path / "r.tsv")
    assert (tmp_path / "r.tsv").read_text() == "\t".join(nov.REGION_COLUMNS) + "\ns.fa\tc1\t380\t421\t21\t1\t1\t1\n"
    nov.write_spectrum(nov.spectrum_frame(counts["depth_hist"]), tmp_path / "sp.tsv")
    assert (tmp_path / "sp.tsv").read_text().split("\n")[:3] == ["depth\tkmers", "1\t50", "2\t4"]
    nov.write_kmers(nov.kmers_frame(np.array([0], np.uint64), [3], 5), tmp_path / "k.tsv")
    assert (tmp_path / "k.tsv").read_text() == "kmer\tdepth\nAAAAA\t3\n"


def test_subcommand_refusals(tmp_path, capsys):
    from panagram_amd.__main__ import main
    fq, fa = tmp_path / "s.fq", tmp_path / "s.fa"
    fq.write_text("@r\nACGT\n+\nIIII\n")
    fa.write_text(">c\nACGT\n")
    for argv, what in ((["novel"], "required"),
                       (["novel", str(tmp_path / "nowhere"), str(fq)], "not an index directory"),
                       (["novel", str(tmp_path), str(tmp_path / "no.fq")], "no sample file"),
                       (["novel", str(tmp_path), str(fq), "--min-count", "0"], "--min-count is 1 to 2^32 - 1"),
                       (["novel", str(tmp_path), str(fq), "--min-count", str(2 ** 32)], "--min-count is 1 to 2^32 - 1"),
                       (["novel", str(tmp_path), str(fq), "--batch-bytes", "0"], "--batch-bytes positive"),
                       (["novel", str(tmp_path), str(fa), "--min-bases", "-1"], "--min-bases not negative"),
                       (["novel", str(tmp_path), str(fa), str(fq), "--regions", str(tmp_path / "r.tsv")], "--regions needs an assembly"),
                       (["novel", str(tmp_path), str(fq), "--min-count", "x"], "invalid int value")):
        with pytest.raises(SystemExit) as ei:
            main(argv)
        assert ei.value.code == 2
        assert what in capsys.readouterr().err, argv
    assert not (tmp_path / "r.tsv").exists()


def test_the_planted_sample_under_the_model():
    """what tests/test_gpu_novel_e2e.py relies on, with the model alone: the FASTA sample's regions are the planted ones, with 500,
    1, 0 and the contig's length as their bases; of the reads at min_count 2 every solid k-mer lies in a planted region and no
    planted error's k-mer is solid"""
    from tests import place_ref as pr
    k = pr.E2E["k"]
    st, spectrum, kmers, regions = NR.e2e_model("fasta", 1, file="s.fa")
    got = [tuple(r) for r in regions[["contig", "start", "kmers", "bases", "left_held", "right_held"]].itertuples(index=False)]
    sub_at = NR.E2E_SUB_AT
    assert got == [("s1", NR.E2E_INS_AT - k + 1, NR.E2E_INSERTION + k - 1, NR.E2E_INSERTION, 1, 1), ("s1", sub_at - k + 1, k, 1, 1, 1),
                   ("s2", NR.e2e_del_at() - k + 1, k - 1, 0, 1, 1), ("s4", 0, NR.E2E_NOVEL_CONTIG - k + 1, NR.E2E_NOVEL_CONTIG, 0, 0)]
    assert st["regions"] == 4 and st["region_bases"] == NR.E2E_INSERTION + 1 + NR.E2E_NOVEL_CONTIG
    assert st["novel_windows"] == int(regions["kmers"].sum()) == st["novel_kmers"] == st["solid_kmers"] and st["error_windows"] == 0
    assert len(NR.e2e_model("fasta", 1, min_bases=2)[3]) == 2
    fasta_keys = set(kmers["kmer"])
    reads, errors = NR.e2e_reads()
    st, spectrum, kmers, none = NR.e2e_model("reads", 2)
    assert none is None and st["regions"] == 0 and st["min_count"] == 2 and st["reads"] == len(reads)
    solid = set(kmers["kmer"])
    print("reads:", st)
    assert solid == fasta_keys  # (every base covered twice or more, and nothing else twice)
    assert len(errors) >= NR.E2E_ERRORS * k // 2 and not solid & set(nov.spell(sorted(errors), k))
    assert st["error_windows"] == len(errors) and st["solid_kmers"] == len(fasta_keys) and st["depth_mode"] >= 4
