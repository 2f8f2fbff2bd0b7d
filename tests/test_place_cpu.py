"""CPU: the numpy model of `place` (tests/place_ref.py) against the oracle's rows, the crafted cases against what they promise,
panagram_amd/place.py's frames and FASTQ batches on hand-made inputs, and the planted end-to-end sample under the model alone."""
import gzip
import os
import re

import numpy as np
import pandas as pd
import pytest

from oracle import pyoracle as po
from panagram_amd import engine, place as pl
from tests import copies_ref as cr
from tests import place_ref as pr
from tests import rows_craft as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_agree_with_the_kernels_header():
    txt = open(os.path.join(ROOT, "panagram_amd", "csrc", "pg_kernels.h")).read()
    const = lambda name: int(re.search(r"constexpr uint32_t %s = (\d+)" % name, txt).group(1))
    assert const("PLACE_CHUNK") == engine.PLACE_CHUNK == pr.CHUNK
    assert const("FASTQ_TILE") == engine.FASTQ_TILE == pr.FASTQ_TILE
    assert const("PROFILE_MAX_GENOMES") == engine.PROFILE_MAX_GENOMES == max(pr.AGREE_N)
    assert const("COPIES_BINS") == engine.COPIES_BINS == cr.BINS


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
def test_model_rows_are_the_oracles_rows():
    """bit g of a row = genome g holds the k-mer: the model's isin against the oracle's anchored rows, N inside the anchor"""
    rng = np.random.default_rng(3)
    k = 15
    a = [pr.rand(rng, 900) + b"N" + pr.rand(rng, 300), pr.rand(rng, 200)]
    b = [pr._substitute(rng, a[0], 0.03), pr.rand(rng, 100)]
    c = [pr.revcomp(a[1]) + pr.rand(rng, 50)]
    genomes = [a, b, c]
    dbs = po.build_bitvec_dbs(genomes, k)
    mine = pr.model_rows(a, genomes, k)
    for contig, bits in zip(a, mine):
        rows = po.anchor_contig(dbs, contig, k, 3)[0]
        _, valid = po.canonical_kmers(contig, k)
        assert np.array_equal(rc.unpack(rows, 3)[valid], bits[valid])
        assert not bits[~valid].any()
        assert bits[valid][:, 0].all()  # the anchor holds its own k-mers
    assert mine[1][:, 2].all() and not mine[1][:, 1].all()


def test_agree_on_a_case_worked_by_hand():
    k = 3
    anchor = [b"ACGTNAC"]           # rows ACG CGT GTN TNA NAC: valid, valid, -, -, valid
    reads = [b"ACG", b"CGT", b"GTA"]  # ACG and CGT are one canonical key (depth 2); TAC = rc(GTA) (depth 1); AC? NAC is invalid
    depths = pr.sample_depths(anchor, pr.joined_reads(reads), k)
    assert depths[0][1].tolist() == [True, True, False, False, False]
    assert depths[0][0].tolist() == [2, 2, 0, 0, 0]
    rows = [rc.pack([[1, 0], [1, 1], [1, 1], [1, 1], [0, 1]])]
    valid, held, col, both = pr.agree(depths, rows, 2, 2, [0, 0, 0], [0, 1, 0], [5, 2, 0])
    assert valid.tolist() == [2, 1, 0] and held.tolist() == [2, 1, 0]
    assert col.tolist() == [[2, 1], [1, 1], [0, 0]] and both.tolist() == [[2, 1], [1, 1], [0, 0]]
    valid, held, col, both = pr.agree(depths, rows, 2, 3, [0], [0], [5])
    assert valid.tolist() == [2] and held.tolist() == [0] and col.tolist() == [[2, 1]] and both.tolist() == [[0, 0]]


@pytest.mark.parametrize("k", pr.AGREE_K)
def test_crafted_agree_case_holds_what_it_promises(k):
    case = pr.agree_case(k)
    anchor, reads, sp = case["anchor"], pr.joined_reads(case["reads"]), case["special"]
    assert len(anchor[1]) == k - 1 and case["nkmers"][1] == 0
    depths = pr.sample_depths(anchor, reads, k)
    d0, v0 = depths[0]
    have = set(d0[v0].tolist())
    for m in pr.AGREE_MIN_COUNTS:  # rows with depth exactly min_count - 1 and min_count, whatever min_count
        assert m - 1 in have and m in have, (k, m)
    assert max(have) >= pr.DEEP
    if k > 6:  # (k = 6: every key occurs all over the anchor and in the random pieces; the depths above are checked all the same)
        for name, d in (("d0", 0), ("d1", 1), ("d2", 2), ("d3", 4), ("d4", 5), ("d5", pr.DEEP), ("never", 0), ("rc_only", 3)):
            assert d0[sp[name][1]] == d and v0[sp[name][1]], (k, name)
        fwd = cr.valid_keys(case["reads"], k)  # the key of rc_only comes from reads that hold its reverse complement only
        kmer = anchor[0][sp["rc_only"][1]:sp["rc_only"][1] + k]
        assert not any(kmer in r for r in case["reads"]) and sum(pr.revcomp(kmer) in r for r in case["reads"]) == 3 and len(fwd)
        assert d0[sp["dup"][1]] == d0[sp["dup2"][1]] == d0[sp["dup_rc"][1]] >= 2  # one key at three rows
    if k % 2 == 0:
        p = sp["pal"][1]
        assert anchor[0][p:p + k] == pr.revcomp(anchor[0][p:p + k]) and d0[p] >= 3 and v0[p]
    # rows the bases outside ACGT take out, on both sides of a chunk edge, and a window that crosses a chunk edge
    assert not v0[3000] and not v0[3000 - k + 1] and v0[3001] and not v0[pr.CHUNK - 3] and not v0[pr.CHUNK - 3 - k + 1]
    assert v0[6000:6200 - k].all()  # lower case is valid
    c, s, e = case["windows"]
    length = (e - s).astype(np.int64)
    for want in (0, 1, pr.CHUNK - 1, pr.CHUNK, pr.CHUNK + 1):
        assert want in length.tolist()
    assert any(ci == 0 and ei == case["nkmers"][0] for ci, ei in zip(c, e)) and {0, 2} <= set(c.tolist())
    assert any(s[i] < e[j] and s[j] < e[i] and c[i] == c[j] for i in range(len(c)) for j in range(i))  # two overlap
    for ci, si, ei in zip(c, s, e):
        assert si <= ei <= case["nkmers"][ci]
    # invalid rows whose bits are set: the planted rows are dense, so some are
    rows = pr.agree_rows(case["nkmers"], 9)
    assert rc.unpack(rows[0], 9)[~v0].any()


# ---------------------------------------------------------------------------
# FASTQ: the model on its own texts, the batches
# ---------------------------------------------------------------------------
def test_fastq_model_on_the_crafted_texts():
    t = pr.fastq_texts()
    assert pr.fastq_model(b"@a\nAC\n+\nII\n@b\nGT\r\n+\nII\n@c\nTT") == (b"ACNGT", 2, 23)
    assert pr.fastq_model(t["zero_bytes"]) == (b"", 0, 0) and pr.fastq_model(t["only_line_feeds"]) == (b"", 0, 0)
    assert pr.fastq_model(t["all_empty"])[0] == b"NN" and pr.fastq_model(t["empty_first"])[0].startswith(b"N")
    j, n, used = pr.fastq_model(t["no_final_lf"])
    assert n == 39 and used < len(t["no_final_lf"]) and t["no_final_lf"][used:].startswith(b"@r39\n")
    assert pr.fastq_model(t["crlf"])[0] == pr.fastq_model(t["lf"])[0] and b"\r" not in pr.fastq_model(t["crlf"])[0]
    assert pr.fastq_model(t["cr_inside"])[0].startswith(b"AC\rGTNACGT\rN")
    for d in (-1, 0, 1):  # the first sequence line's last base at offset tile - 2 + d, its line feed right behind
        text = t[f"tile_edge{d:+d}"]
        assert text.index(b"\n", 3) == pr.FASTQ_TILE + d
    r3 = t["cut_line3"].index(b"@r3\n")  # records 0..2 are whole, the cut falls inside record 3
    for name, line in (("cut_line0", 0), ("cut_line1", 1), ("cut_line2", 2), ("cut_line3", 3), ("cut_after_line2", 3)):
        j, n, used = pr.fastq_model(t[name])
        assert n == 3 and used == r3 < len(t[name]) and t[name][r3:].count(b"\n") == line, name
    assert pr.fastq_model(t["many_short"])[1] == 70_000 and len(pr.fastq_model(t["many_short"])[0]) == 4 * 70_000 - 1
    for name, text in t.items():
        assert not pr.fastq_malformed(text), name
    bad = pr.fastq_malformed_texts()
    assert bad["no_at"][1] == [150] and bad["no_plus"][1] == [0] and bad["empty_header"][1] == [3] and len(bad["shifted"][1]) > 100
    assert pr.as_packed(b"acgtNrXT\r") == b"ACGTNNNTN"


def _drain(path, batch_bytes):
    """every batch consumed as the model says: (the joined sequences, reads, batches)"""
    fb = pl.FastqBatches(path, batch_bytes)
    joined, reads, nb = [], 0, 0
    for buf in fb:
        j, n, used = pr.fastq_model(buf)
        if n:
            joined.append(j)
        reads += n
        nb += 1
        fb.advance(used)
    return b"N".join(joined), reads, nb


def test_fastq_batches(tmp_path):
    rng = np.random.default_rng(9)
    reads = [pr.rand(rng, int(n)) for n in rng.integers(1, 300, 200)]
    text = pr.fastq_text(reads)
    want = b"N".join(reads)
    plain, gz, nolf, torn = (str(tmp_path / n) for n in ("a.fq", "b.fq.gz", "c.fq", "d.fq"))
    open(plain, "wb").write(text)
    with gzip.open(gz, "wb") as f:
        f.write(text)
    open(nolf, "wb").write(text[:-1])
    open(torn, "wb").write(text[:text.rindex(b"\n+\n")])  # (the last record ends with its sequence line)
    for path in (plain, gz, nolf):
        for bb in (len(text) + 5, len(text), 5000, 700, 64):  # (64: most batches hold no whole record, the tail grows)
            j, n, nb = _drain(path, bb)
            assert (j, n) == (want, 200), (path, bb)
            assert nb >= min(len(text) // bb, 1)
    assert _drain(plain, 5000)[2] > 5  # a tail was carried over
    with pytest.raises(ValueError, match="not a whole FASTQ record"):
        _drain(torn, 5000)
    empty = str(tmp_path / "e.fq")
    open(empty, "wb").close()
    assert _drain(empty, 100) == (b"", 0, 0)
    fb = pl.FastqBatches(plain, 1000)
    with pytest.raises(RuntimeError, match="advance"):
        for _ in fb:
            pass
    with pytest.raises(ValueError):
        pl.FastqBatches(plain, 0)


# ---------------------------------------------------------------------------
# frames
# ---------------------------------------------------------------------------
def test_frames_ties_nan_dot_selection_and_sums():
    names = ["A", "B", "C"]
    bins = pd.DataFrame({"chrom": ["c1", "c1", "c2", "c2"], "start": [0, 10, 0, 10], "end": [10, 20, 10, 15]})
    valid = [10, 10, 10, 0]
    held = [4, 6, 0, 0]
    col = [[4, 4, 8], [6, 3, 6], [0, 0, 0], [0, 0, 0]]
    both = [[2, 2, 4], [6, 3, 0], [0, 0, 0], [0, 0, 0]]
    main, matrix, summary = pl.frames(bins, valid, held, col, both, names)
    # bin 0: A 2/6, B 2/6, C 4/8 -> C, then A (the tie goes to the genome earlier in the index)
    # bin 1: A 6/6, B 3/6, C 0/12 -> A, B;  bin 2: col = held = 0 -> every Jaccard NaN;  bin 3: no valid row
    assert main.columns.tolist() == pl.MAIN_COLUMNS
    assert main["best"].tolist() == ["C", "A", ".", "."] and main["second"].tolist() == ["A", "B", ".", "."]
    assert np.allclose(main["best_jaccard"][:2], [0.5, 1.0]) and np.allclose(main["second_jaccard"][:2], [1 / 3, 0.5])
    assert main["best_jaccard"][2:].isna().all() and main["second_jaccard"][2:].isna().all()
    assert main["valid"].tolist() == valid and main["held"].tolist() == held and main["end"].tolist() == [10, 20, 10, 15]
    assert matrix.columns.tolist() == names and matrix.index.tolist() == [("c1", 0), ("c1", 10), ("c2", 0), ("c2", 10)]
    assert np.allclose(matrix.to_numpy()[:2], [[1 / 3, 1 / 3, 0.5], [1.0, 0.5, 0.0]]) and np.isnan(matrix.to_numpy()[2:]).all()
    assert summary.columns.tolist() == pl.SUMMARY_COLUMNS
    assert summary["col"].tolist() == [10, 7, 14] and summary["both"].tolist() == [8, 5, 4] and summary["bins_best"].tolist() == [1, 0, 1]
    assert np.allclose(summary["jaccard"], [8 / 12, 5 / 12, 4 / 20]) and np.allclose(summary["cont_g"], [0.8, 5 / 7, 4 / 14])
    assert np.allclose(summary["cont_s"], [0.8, 0.5, 0.4])
    # a selection, in index order whatever the order given; the tie of bin 0 is now between A and B: A
    main, matrix, summary = pl.frames(bins, valid, held, col, both, names, ["B", "A"])
    assert matrix.columns.tolist() == ["A", "B"] and main["best"].tolist() == ["A", "A", ".", "."] and main["second"].tolist()[:2] == ["B", "B"]
    assert summary["genome"].tolist() == ["A", "B"] and summary["bins_best"].tolist() == [2, 0]
    one = pl.frames(bins, valid, held, col, both, names, ["C"])[0]
    assert one["best"].tolist() == ["C", "C", ".", "."] and one["second"].tolist() == ["."] * 4 and one["second_jaccard"].isna().all()
    with pytest.raises(KeyError, match="nobody"):
        pl.frames(bins, valid, held, col, both, names, ["nobody"])
    # 0 / 0 is NaN, x / 0 never happens (both <= col, both <= held)
    j, cg, cs = pl.ratios([0, 5, 0], [0, 0, 0], [0, 0, 7])
    assert np.isnan(j[0]) and j[1] == 0 and j[2] == 0 and np.isnan(cg[0]) and np.isnan(cg[2]) and np.isnan(cs[0]) and np.isnan(cs[1])
    # no bin at all
    none = pl.frames(bins.iloc[:0], [], [], np.zeros((0, 3)), np.zeros((0, 3)), names)
    assert len(none[0]) == 0 and none[1].shape == (0, 3) and none[2]["col"].tolist() == [0, 0, 0] and none[2]["jaccard"].isna().all()


def test_summary_file_and_depth_mode(tmp_path):
    assert pl.depth_mode([100, 3, 9, 9, 2]) == 2 and pl.depth_mode([5, 0, 0]) == 0 and pl.depth_mode(np.zeros(64)) == 0
    bins = pd.DataFrame({"chrom": ["c"], "start": [0], "end": [9]})
    main, matrix, summary = pl.frames(bins, [9], [3], [[3, 0]], [[3, 0]], ["A", "B"])
    stats = dict(reads=12, read_bases=1200, hits=777, depth_mode=8, min_count=2)
    p, m, o = (str(tmp_path / n) for n in ("s.tsv", "m.tsv", "o.tsv"))
    pl.write_summary(summary, stats, p)
    pl.write_matrix(matrix, m)
    pl.write_main(main, o)
    lines = open(p).read().split("\n")
    assert lines[:5] == ["# reads\t12", "# read_bases\t1200", "# hits\t777", "# depth_mode\t8", "# min_count\t2"]
    assert lines[5] == "\t".join(pl.SUMMARY_COLUMNS) and lines[6] == "A\t3\t3\t1.000000\t1.000000\t1.000000\t1" and lines[7].startswith("B\t0\t0\t0.000000\tNaN\t0.000000\t0")
    assert open(m).read() == "chrom\tstart\tA\tB\nc\t0\t1.000000\t0.000000\n"
    assert open(o).read() == "\t".join(pl.MAIN_COLUMNS) + "\nc\t0\t9\t9\t3\tA\t1.000000\tB\t0.000000\n"


# ---------------------------------------------------------------------------
# the planted end-to-end sample, under the model alone
# ---------------------------------------------------------------------------
def test_planted_sample_calls_its_donors_under_the_model():
    main, matrix, summary, stats = pr.e2e_model()
    p = pr.E2E
    donors = pr.e2e_donor_bins()
    assert {d for _, _, d in donors} == {"B", "C"} and len(donors) >= 6
    got = {(c, s): b for c, s, b in zip(main["chrom"], main["start"], main["best"])}
    for chrom, start, donor in donors:
        assert got[(chrom, start)] == donor, (chrom, start, donor, got[(chrom, start)])
    assert len(main) == sum(-(-(n - p["k"] + 1) // p["bin_size"]) for n in p["contig_lens"])
    assert stats["reads"] == len(pr.e2e_reads()) and stats["depth_mode"] >= 5
    assert set(summary["genome"]) == set(pr.E2E_NAMES) and summary["bins_best"].sum() == len(main)
    # a selection without the donors: the anchor is all that is left to call
    only = pr.e2e_model(genomes=["A"])[0]
    assert set(only["best"]) == {"A"}
