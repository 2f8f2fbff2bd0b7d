"""GPU: `intros` on indexes written by Index.run().  Genome.kmer_similarity_bins (bitmap inflated into HBM, binned by
k_bin_colsums) against the restatement of bitmap_to_bins (tests/intros_ref.py) on rows taken from gzip.decompress of the
same bitmap files — N = 3, 9, 40, 70, 130 (one-, two-, five-, nine- and seventeen-byte rows), steps 1 to 300 read from bitmap.1 and from
low-resolution bitmaps of step 100 and 50, bins that do and do not divide by the step, --rmf, a keep mask over two and
three 32-bit words, batches split per chromosome.  Then a planted introgression: a 20 kb segment of a WILD genome copied
into a CULT genome is called, and the 2-way (REFA) and --urf BEDs equal the restated pipeline byte for byte."""
import os
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from oracle import pyoracle as po
from tests import intros_ref as ref

pytestmark = pytest.mark.gpu

K = 21
CASES = [  # (genomes, low-resolution step, contig lengths, keep mask columns)
    (3, 100, [12000, 5000, 900], [0, 2]),
    (9, 50, [11000, 4000, 15], [0, 8]),
    (40, 100, [9000, 3500], [1, 33]),
    (70, 50, [6000, 2500], [1, 33, 66]),
    (130, 100, [4000, 1500], [1, 129]),  # (17-byte rows: k_bin_colsums<0>, the keep mask in words 0 and 4)
]
STEPS = [1, 7, 100, 200, 300]
BINS = [1000, 1050, 5000]


def write_samples(tmp, genomes, names, chroms):
    rows = ["name\tfasta"]
    for nm, g in zip(names, genomes):
        fa = tmp / f"{nm}.fa"
        fa.write_bytes(po.fasta_text(chroms, [po.codes_to_ascii(c) for c in g]))
        rows.append(f"{nm}\t{fa}")
    (tmp / "samples.tsv").write_text("\n".join(rows) + "\n")
    return str(tmp / "samples.tsv")


@pytest.fixture(scope="module", params=CASES, ids=[f"N{c[0]}_low{c[1]}" for c in CASES])
def built(request, tmp_path_factory):
    from panagram_amd import index as pidx
    n, low, lens, keep = request.param
    tmp = tmp_path_factory.mktemp(f"intros_n{n}")
    chroms = [f"chr{i + 1}" for i in range(len(lens))]
    samples = write_samples(tmp, po.synth_genomes(n, lens, 0.02, 17 + n), [f"g{i}" for i in range(n)], chroms)
    out = str(tmp / "idx")
    pidx.Index(samples, prefix=out, k=K, anchor_genomes=["g0"], lowres_step=low).run()
    return out, n, low, keep


def restated(idx, g, chrom, step, bin_size, omit, keep, cache):
    key = (chrom, step)
    if key not in cache:
        cache[key] = ref.query_frame(g.prefix, idx.genome_names, g.chrs, idx.steps, chrom, step)
    fr = cache[key]
    if len(fr) == 0:
        return None
    return ref.bitmap_to_bins(fr, bin_size, omit, keep)


def test_kmer_similarity_bins_parity(built):
    from panagram_amd import index as pidx
    out, n, low, keep_cols = built
    idx = pidx.Index(out, mode="r")
    try:
        assert idx.steps == (1, low)
        g = idx["g0"]
        g.load_chrs()
        names = list(idx.genome_names)
        keep = [names[i] for i in keep_cols]
        cache, checked = {}, 0
        for step in STEPS:
            for bin_size in BINS:
                for omit, kp in ((False, None), (True, None), (False, keep), (True, keep)):
                    got = g.kmer_similarity_bins(step=step, bin_size=bin_size, omit_fixed=omit, keep=kp)
                    assert list(got) == list(g.chrs.index)
                    for chrom, fr in got.items():
                        want = restated(idx, g, chrom, step, bin_size, omit, kp, cache)
                        if want is None:
                            assert fr.shape == (n, 0) and list(fr.index) == names
                            continue
                        pd.testing.assert_frame_equal(fr, want, obj=f"{chrom} step {step} bin {bin_size} rmf {omit} keep {kp}")
                        checked += 1
        assert checked >= len(STEPS) * len(BINS) * 4 * 2
        # the edge cases occur: NaN (all-zero sums) or 1.0 fills somewhere, and bins where not every genome is 1.0
        full = g.kmer_similarity_bins(step=1, bin_size=1000, omit_fixed=True)
        assert any((fr < 1).any().any() for fr in full.values())
    finally:
        idx.close()


def test_batches_split_per_chromosome(built):
    from panagram_amd import index as pidx
    out, n, low, keep_cols = built
    idx = pidx.Index(out, mode="r")
    try:
        g = idx["g0"]
        g.load_chrs()
        keep = [list(idx.genome_names)[i] for i in keep_cols]
        for step in (1, 2 * low):
            whole = g.kmer_similarity_bins(step=step, bin_size=1050, omit_fixed=True, keep=keep)
            g.similarity_budget = 1  # every chromosome a launch of its own
            try:
                split = g.kmer_similarity_bins(step=step, bin_size=1050, omit_fixed=True, keep=keep)
            finally:
                del g.similarity_budget
            chroms = list(g.chrs.index)[::-1]  # a subset in another order: the same frames, in the order asked
            part = g.kmer_similarity_bins(chroms[:2], step=step, bin_size=1050, omit_fixed=True, keep=keep)
            assert list(part) == chroms[:2]
            for c in whole:
                pd.testing.assert_frame_equal(split[c], whole[c])
                if c in part:
                    pd.testing.assert_frame_equal(part[c], whole[c])
    finally:
        idx.close()


# ---------------------------------------------------------------------------
# a planted introgression
# ---------------------------------------------------------------------------
GROUPS = {"REF1": "REF", "REF2": "REF", "CULT1": "CULT", "CULT2": "CULT", "WILD1": "WILD", "WILD2": "WILD"}
LENS, SEG = [100000, 30000], (40000, 60000)


def _mutate(seqs, d, seed):
    r = np.random.default_rng(seed)
    out = []
    for b in seqs:
        mut = r.random(len(b)) < d
        out.append(np.where(mut, (b + r.integers(1, 4, len(b), dtype=np.uint8)) & 3, b).astype(np.uint8))
    return out


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    from panagram_amd import index as pidx
    tmp = tmp_path_factory.mktemp("planted")
    rng = np.random.default_rng(11)
    base = [rng.integers(0, 4, L, dtype=np.uint8) for L in LENS]
    wild = _mutate(base, 0.12, 1)
    seqs = {"REF1": _mutate(base, 0.003, 2), "REF2": _mutate(base, 0.003, 3), "CULT1": _mutate(base, 0.003, 4),
            "CULT2": _mutate(base, 0.003, 5), "WILD1": _mutate(wild, 0.003, 6), "WILD2": _mutate(wild, 0.003, 7)}
    seqs["CULT1"][0][SEG[0]:SEG[1]] = seqs["WILD1"][0][SEG[0]:SEG[1]]  # the donor's segment
    samples = write_samples(tmp, list(seqs.values()), list(seqs), ["chr1", "chr2"])
    out = tmp / "idx"
    pidx.Index(samples, prefix=str(out), k=K, anchor_genomes=["CULT1", "REF1"]).run()
    tsv = tmp / "groups.tsv"
    tsv.write_text("name\tgroup\n" + "".join(f"{n}\t{g}\n" for n, g in GROUPS.items()))
    return tmp, out, tsv


def _restated_beds(out, genome, anchor, comp, thr, binlen, step, urf=False, gnm=None, sft=None, ssz=5, rmf=False):
    from panagram_amd import index as pidx
    idx = pidx.Index(str(out), mode="r")
    try:
        g = idx[genome]
        g.load_chrs()
        frames = {c: ref.bitmap_to_bins(ref.query_frame(g.prefix, idx.genome_names, g.chrs, idx.steps, c, step), binlen, rmf)
                  for c in g.chrs.index}
    finally:
        idx.close()
    sims = ref.similarities(list(frames.values()), 3.0) if gnm else None
    beds = {}
    for c, fr in frames.items():
        pre = ref.preprocess(fr, sims, gnm, sft, ssz, False)
        calls = (pre.loc[anchor] < thr).astype(int) if urf else ref.calls_3way_or_2way(pre, GROUPS, comp, thr)
        name = comp if urf or comp != "REF" else "REFA"
        beds[f"{anchor}_{c}_{name}.bed"] = ref.bed_text(calls, binlen, c, name)
    return beds


def _read(d):
    return {p.name: p.read_text() for p in sorted(Path(d).iterdir())}


def test_planted_introgression_is_called(planted):
    from panagram_amd.__main__ import main
    tmp, out, tsv = planted
    calls = tmp / "calls3"
    assert main(["intros", "call", "--idx", str(out), "--tsv", str(tsv), "--out", str(calls), "--anc", "CULT1",
                 "--cmp", "WILD", "--thr", "0.2", "--bin", "2000", "--stp", "1"]) == 0
    raw = calls / "calls3_0.2" / "raw"
    assert sorted(os.listdir(raw)) == ["CULT1_chr1_WILD.bed", "CULT1_chr2_WILD.bed"]
    recs = [line.split("\t") for line in (raw / "CULT1_chr1_WILD.bed").read_text().splitlines()]
    assert recs, "the planted segment was not called"
    covered = set()
    for c, s, e, name in recs:
        assert c == "chr1" and name == "WILD_intro"
        s, e = int(s), int(e)
        assert SEG[0] - 2000 <= s and e < SEG[1] + 2000, (s, e)  # nothing far from the segment
        covered.update(range(s // 2000, (e + 1) // 2000))
    assert set(range(SEG[0] // 2000, SEG[1] // 2000)) <= covered  # the segment at bin resolution
    assert (raw / "CULT1_chr2_WILD.bed").read_text() == ""
    assert _read(raw) == _restated_beds(out, "CULT1", "CULT1", "WILD", 0.2, 2000, 1)


def test_refa_and_urf_equal_restated_pipeline(planted):
    from panagram_amd.__main__ import main
    tmp, out, tsv = planted
    calls = tmp / "calls2"
    assert main(["intros", "call", "--idx", str(out), "--tsv", str(tsv), "--out", str(calls), "--anc", "CULT1",
                 "--cmp", "REF", "--thr", "0.5", "--bin", "2000", "--stp", "1", "--gnm", "-1", "--sft", "mean", "--ssz", "3",
                 "--rmf"]) == 0
    got = _read(calls / "calls2_0.5" / "raw")
    assert got == _restated_beds(out, "CULT1", "CULT1", "REF", 0.5, 2000, 1, gnm=-1, sft="mean", ssz=3, rmf=True)
    assert got["CULT1_chr1_REFA.bed"]
    urf = tmp / "urf"
    assert main(["intros", "call", "--idx", str(out), "--tsv", str(tsv), "--out", str(urf), "--anc", "CULT1",
                 "--cmp", "REF", "--urf", "--ref", "REF1", "--thr", "0.5", "--bin", "2000", "--stp", "1"]) == 0
    got = _read(urf / "urf_0.5" / "raw")
    assert got == _restated_beds(out, "REF1", "CULT1", "REF", 0.5, 2000, 1, urf=True)
    assert sorted(got) == ["CULT1_chr1_REF.bed", "CULT1_chr2_REF.bed"] and got["CULT1_chr1_REF.bed"]


def test_config_sweep_writes_every_threshold(planted):
    from panagram_amd.__main__ import main
    tmp, out, tsv = planted
    cfg = tmp / "intros.yaml"
    cfg.write_text(f"""general:
  output_dir: {tmp / 'sweep'}
  index_dir: {out}
  tsv: {tsv}
  bin: 2000
  ref: REF1
  threads: 4
calling:
  run: true
  grp: null
  anc: [CULT1]
  chr: null
  cmp: [WILD]
  thr: [0.2]
  stp: 100
  gnm: null
  trm: 3
  sft: null
  ssz: null
  urf: false
  rmf: false
  rmu: null
  ogrp: null
  edg: false
  vis: false
postprocessing:
  run: false
scoring:
  run: false
""")
    assert main(["intros", str(cfg), "--sweep"]) == 0
    dirs = sorted(p.name for p in (tmp / "sweep").iterdir() if p.is_dir())
    assert len(dirs) == 18 and "sweep_0.0" in dirs and "sweep_0.68" in dirs
    for d in dirs:
        assert sorted(os.listdir(tmp / "sweep" / d / "raw")) == ["CULT1_chr1_WILD.bed", "CULT1_chr2_WILD.bed"]
    assert (tmp / "sweep" / "intro_config.yaml").read_text() == cfg.read_text()
