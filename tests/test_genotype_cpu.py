"""CPU: the host side of `genotype` — the piece cutter and the piece sum of panagram_amd/csrc/pg_genotype_host.h against the numpy
model (tools/genotype_stitch_check.cpp, compiled without sanitizer flags and run), the call rule, the frames and the VCF lines of
panagram_amd/genotype.py against tests/genotype_ref.py — and the model itself on the planted sample, whose genotypes follow by
construction: reads of A call every site 0/0, reads of B 1/1, both 0/1, a mosaic by its donor."""
import os
import shutil
import subprocess

import numpy as np
import pandas as pd
import pytest

from panagram_amd import genotype as gt
from panagram_amd import synteny
from tests import genotype_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW_COUNTS = (0, 1, 63, 64, 65, 256, 257, 4097)


@pytest.mark.parametrize("n", WINDOW_COUNTS)
def test_the_piece_cutter_covers_every_window_once(n):
    for p0 in (0, 5, 1 << 33):
        pieces = gr.cut(p0, p0 + n)
        assert len(pieces) == (n + gr.PIECE - 1) // gr.PIECE
        got = [p for s, m in pieces for p in range(s, s + m)]
        assert got == list(range(p0, p0 + n))
        assert all(1 <= m <= gr.PIECE for _, m in pieces) and all(m == gr.PIECE for _, m in pieces[:-1])


def test_window_interval_by_the_definition():
    """every window that overlaps the allele; for a junction the k - 1 windows that hold both its neighbours"""
    for k in (1, 2, 6, 21):
        for L in (0, 1, k - 1, k, k + 1, 3 * k + 2):
            if L < 0:
                continue
            for s in range(L + 1):
                for l in range(L - s + 1):
                    nk = max(L - k + 1, 0)
                    want = [p for p in range(nk) if (p < s + l and p + k > s if l else p <= s - 1 and p + k > s)]
                    p0, p1 = gr.window_interval(L, k, s, l)
                    assert list(range(p0, p1)) == want, (k, L, s, l)
    k = 21
    assert gr.window_interval(1000, k, 500, 0) == (480, 500) and gr.window_interval(1000, k, 500, 1) == (480, 501)  # k - 1 and k windows
    assert gr.window_interval(1000, k, 0, 0)[0] == gr.window_interval(1000, k, 0, 0)[1]
    assert gr.window_interval(1000, k, 1000, 0)[0] == gr.window_interval(1000, k, 1000, 0)[1]
    assert gr.window_interval(k - 1, k, 3, 5)[0] == gr.window_interval(k - 1, k, 3, 5)[1]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_the_hosts_cutter_and_piece_sum_equal_the_model(tmp_path):
    exe = str(tmp_path / "genotype_stitch_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tools", "genotype_stitch_check.cpp")], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("ok:"), (p.returncode, p.stdout, p.stderr)
    # ranges with the window counts above, at every k of the GPU tests, and the edges: the program's sums of partials made up from
    # (range, piece, windows) against the same sums over the model's pieces
    cases = []
    for k in (6, 21, 31, 32):
        for n in WINDOW_COUNTS[1:]:
            cases += [(6000, k, 700, n - k + 1)] if n >= k - 1 else [(6000, k, n, 0)]  # (a junction n bases in has n windows)
        cases += [(6000, k, 0, 0), (6000, k, 6000, 0), (6000, k, 2, 3), (6000, k, 5998, 2), (k - 1, k, 0, k - 1), (k, k, 0, k), (k, k, 3, 0),
                  (70000, k, 0, 70000), (70000, k, 100, 65536)]
    (tmp_path / "cases.txt").write_text("".join("%d %d %d %d\n" % c for c in cases))
    p = subprocess.run([exe, str(tmp_path / "cases.txt")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr)
    got = [[int(x) for x in ln.split()] for ln in p.stdout.splitlines()]
    assert len(got) == len(cases)
    counts = set()
    for i, ((L, k, s, l), g) in enumerate(zip(cases, got)):
        p0, p1 = gr.window_interval(L, k, s, l)
        pieces = gr.cut(p0, p1)
        inf = [(7 * j + i) % (n + 1) for j, (_, n) in enumerate(pieces)]
        want = [p0, p1, len(pieces), p1 - p0, sum(inf), sum(x // 2 for x in inf), sum((1 << 33) + j * x for j, x in enumerate(inf))]
        assert g == want, (cases[i], g, want)
        counts.add(p1 - p0)
    assert set(WINDOW_COUNTS) <= counts and 65536 + 20 in counts
    assert [g[2] for (L, k, s, l), g in zip(cases, got) if (k, l) == (21, 65536)] == [1025]  # no wave loops: 1 025 pieces


def test_the_call_rule_on_a_hand_made_table():
    F = 0.5
    table = [  # ref inf, ref seen, alt inf, alt seen -> GT, flag
        ((0, 0, 10, 10), ("./.", "uninformative")), ((10, 10, 0, 0), ("./.", "uninformative")), ((0, 0, 0, 0), ("./.", "uninformative")),
        ((10, 10, 10, 0), ("0/0", "")), ((10, 0, 10, 10), ("1/1", "")), ((10, 10, 10, 10), ("0/1", "")), ((10, 0, 10, 0), ("./.", "neither")),
        ((10, 5, 10, 4), ("0/0", "")),   # seen == F * inf exactly: present; one below: absent
        ((10, 4, 10, 5), ("1/1", "")), ((4, 2, 6, 3), ("0/1", "")), ((21, 10, 21, 11), ("1/1", "")), ((21, 5, 21, 5), ("./.", "neither")),
        ((1, 1, 1, 0), ("0/0", "")), ((1, 0, 1, 0), ("./.", "neither"))]
    for args, want in table:
        assert gr.call(*args, F) == want, args
    cols = np.array([a for a, _ in table], np.int64).T
    got = gt.call(*cols, F)
    assert list(zip(got[0].tolist(), got[1].tolist())) == [w for _, w in table]
    # F = 1: every informative k-mer must be seen
    ones = [((10, 10, 10, 9), ("0/0", "")), ((10, 9, 10, 9), ("./.", "neither")), ((3, 3, 2, 2), ("0/1", "")), ((0, 0, 2, 2), ("./.", "uninformative"))]
    for args, want in ones:
        assert gr.call(*args, 1.0) == want
    got = gt.call(*np.array([a for a, _ in ones], np.int64).T, 1.0)
    assert list(zip(got[0].tolist(), got[1].tolist())) == [w for _, w in ones]
    for bad in (0, 0.0, -0.1, 1.0001, 2):
        with pytest.raises(ValueError, match="min_frac"):
            gt.check_min_frac(bad)
    assert gt.check_min_frac(1) == 1.0 and gt.check_min_frac(1e-9) == 1e-9
    with pytest.raises(ValueError, match="min_count"):
        gt.check_min_count(0)


@pytest.fixture(scope="module")
def model():
    return {name: gr.e2e_model(21, name) for name in gr.samples()}


def test_the_planted_sites_are_the_variants(model):
    """the numpy models of runs and variants find every planted edit where it was planted; the two SNPs five bases apart are one mnp"""
    a, b, edits = gr.planted()
    planted = [(gr.E2E_CHROMS[c], q, n, alt.decode()) for c, es in enumerate(edits) for q, n, alt in es if not gr.is_hard(c, q)]
    rows = model["reads_a"]["rows"]
    assert [(r[0], r[1], r[2], r[9]) for r in rows if not gr.is_hard(gr.E2E_CHROMS.index(r[0]), r[1])] == planted
    hard = [r for r in rows if gr.is_hard(gr.E2E_CHROMS.index(r[0]), r[1])]
    assert [r[7] for r in hard] == ["mnp", "ins"] and len(rows) == len(planted) + 2 >= 140
    assert {r[7] for r in rows} == {"snp", "mnp", "ins", "del"}
    assert max(r[2] for r in rows) > 250 and max(r[5] for r in rows) > 80  # deletions of up to 300 bases, insertions of up to 90


@pytest.mark.parametrize("sample", sorted(gr.samples()))
def test_the_model_calls_the_planted_truth(model, sample):
    m = model[sample]
    rows = m["rows"]
    left_out = [r for r in rows if r[16] == "./."]
    print(sample, "sites", len(rows), "left out", len(left_out), {g: sum(1 for r in rows if r[16] == g) for g in gr.GENOTYPES})
    assert len(left_out) <= 0.05 * len(rows)   # the condition the GPU tests inherit (on these genomes: none)
    assert left_out == []
    for r, want in gr.truth_rows(m, sample):
        assert r[16] == want and r[17] == "", r
    assert m["min_count"] == 2 and m["reads"] > 4000
    if sample == "mosaic":
        gts = [r[16] for r in rows]
        assert gts.count("0/0") > 50 and gts.count("1/1") > 50


def test_an_assembly_gives_the_same_genotypes(model):
    fa = gr.e2e_model(21, "mosaic", fasta=True)
    assert fa["min_count"] == 1 and fa["reads"] == 3
    assert [r[16] for r in fa["rows"]] == [r[16] for r in model["mosaic"]["rows"]]


def test_frames_table_and_summary_are_the_models(model):
    for name, m in model.items():
        table, summary = gt.frames(m["frame"], *m["support"], gr.E2E_MIN_FRAC)
        assert list(table.columns) == gt.FRAME_COLUMNS and gt.TABLE_COLUMNS == gr.TABLE_COLUMNS
        assert gt.table_text(table) == gr.table_text(m["rows"]), name
        st = gt.stats(table, *m["support"], m["reads"], m["hits"], m["min_count"], gr.E2E_MIN_FRAC)
        assert gt.summary_text(summary, st) == gr.summary_text(m["rows"], m["reads"], m["hits"], *m["support"], m["min_count"], gr.E2E_MIN_FRAC)
        assert st["sites"] == len(m["rows"]) == st["callable"] and list(st) == gt.STAT_NAMES
    # flags and empty fields in the text: a site without informative k-mers, one with neither allele
    frame = model["reads_a"]["frame"].iloc[:3].copy()
    frame.attrs = {"anchor": model["reads_a"]["frame"].attrs["anchor"][:3]}
    ref = ([5, 5, 5], [0, 4, 4], [0, 0, 4], [0, 0, 9])
    alt = ([5, 5, 5], [4, 4, 4], [0, 0, 0], [0, 0, 0])
    table, summary = gt.frames(frame, ref, alt, 0.5)
    assert table["GT"].tolist() == ["./.", "./.", "0/0"] and table["flag"].tolist() == ["uninformative", "neither", ""]
    assert table["ref_depth"].tolist() == [".", "0.00", "2.25"] and table["alt_depth"].tolist() == ["0.00"] * 3
    rows = gr.table_rows([tuple(r) for r in frame[gr.TABLE_COLUMNS[:10]].itertuples(index=False)], ref, alt, 0.5)
    assert gt.table_text(table) == gr.table_text(rows)
    assert gt.table_text(table).splitlines()[3].split("\t")[-1] == "-"
    assert gt.stats(table, ref, alt, 0, 0, 2, 0.5)["callable"] == 2
    with pytest.raises(ValueError, match="one entry per variant"):
        gt.frames(frame, ([1], [1], [1], [1]), alt, 0.5)


def test_vcf_lines_carry_the_call(model):
    m = model["mosaic"]
    a, _, _ = gr.planted()
    lens_a = dict(zip(gr.E2E_CHROMS, (len(c) for c in a)))
    table, _ = gt.frames(m["frame"], *m["support"], gr.E2E_MIN_FRAC)
    lines = gt.vcf_lines(table, lens_a, "mine")
    base = synteny.vcf_lines(m["frame"], lens_a, "mine")
    head = [ln for ln in lines if ln.startswith("#")]
    assert lines[:len(head)] == head and head[0] == "##fileformat=VCFv4.2"
    assert [ln for ln in head if ln not in gt.FORMAT_LINES] == [ln for ln in base if ln.startswith("#")]  # synteny's header, two lines more
    assert head[-1].split("\t")[-2:] == ["FORMAT", "mine"] and head[-3:-1] == gt.FORMAT_LINES
    declared = {ln.split("ID=")[1].split(",")[0] for ln in head if ln.startswith("##FORMAT")}
    assert declared == {"GT", "RK", "AK"}
    body = [ln.split("\t") for ln in lines[len(head):]]
    assert [f[:8] for f in body] == [ln.split("\t")[:8] for ln in base[len(head) - 2:]]  # the variant's own fields are synteny's
    assert [(f[0], f[1], f[3], f[4], f[8], f[9]) for f in body] == gr.vcf_body(m["rows"], m["anchors"])
    for f, r in zip(body, m["rows"]):
        assert len(f) == 10 and a[gr.E2E_CHROMS.index(f[0])][int(f[1]) - 1:int(f[1]) - 1 + len(f[3])].decode() == f[3]  # REF is A's text
        assert f[9].split(":")[0] == r[16]


def test_allele_ranges_number_the_whole_assemblies(model):
    frame = model["reads_a"]["frame"]
    ra, rb = gt.allele_ranges(frame, ["chr0"] + gr.E2E_CHROMS, gr.E2E_CHROMS)
    assert ra[0].dtype == np.uint32 and ra[1].dtype == np.uint64 and ra[2].dtype == np.uint64
    assert ra[0].tolist() == [gr.E2E_CHROMS.index(c) + 1 for c in frame["chrA"]] and rb[0].tolist() == [gr.E2E_CHROMS.index(c) for c in frame["chrB"]]
    assert ra[1].tolist() == frame["posA"].tolist() and rb[2].tolist() == frame["altLen"].tolist()
    with pytest.raises(ValueError, match="chr3"):
        gt.allele_ranges(frame, gr.E2E_CHROMS[:2], gr.E2E_CHROMS)
    empty = frame.iloc[:0]
    assert [len(x) for side in gt.allele_ranges(empty, [], []) for x in side] == [0] * 6
