"""CPU: the host side of `intros` — bin geometry, the binned frame's division and edge cases, preprocessing, thresholds,
`merged` and BED records, output layout, config.yaml and --sweep, and every input error — against the restatement in
tests/intros_ref.py, on hand-built frames and rows."""
import os
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest

from panagram_amd import introgressions as it
from panagram_amd.index import Genome
from tests import intros_ref as ref


# ---------------------------------------------------------------------------
# bin geometry and the frame of one chromosome
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("size", [1, 999, 1000, 12345, 20000])
@pytest.mark.parametrize("step,bin_size", [(1, 1000), (7, 1000), (100, 1050), (300, 1000), (200, 5000), (300, 100),
                                           (1000, 1000), (7, 3)])
def test_bin_geometry_matches_positions(size, step, bin_size):
    b, s, e = Genome.similarity_bin_geometry(size, step, bin_size)
    pos = np.arange(0, size, step)
    want_b = np.unique(pos // bin_size)
    assert list(b) == list(want_b)
    for bi, si, ei in zip(b, s, e):
        js = np.flatnonzero(pos // bin_size == bi)
        assert (si, ei) == (js[0], js[-1] + 1)
    assert (e[-1] if len(e) else 0) == len(pos)


def test_bin_geometry_empty_chromosome():
    b, s, e = Genome.similarity_bin_geometry(0, 100, 1000)
    assert len(b) == len(s) == len(e) == 0


def _sums(bits, bins_of_row, nb, omit_fixed, keep_idx):
    rows = bits.copy()
    if keep_idx is not None:
        none = rows[:, keep_idx].sum(axis=1) == 0
        rows[np.ix_(none, keep_idx)] = 1
    take = ~(omit_fixed & rows.all(axis=1))
    cs = np.zeros((nb, bits.shape[1]), np.uint64)
    kept = np.zeros(nb, np.uint64)
    for b in range(nb):
        m = (bins_of_row == b) & take
        cs[b] = rows[m].sum(axis=0)
        kept[b] = m.sum()
    return cs, kept


@pytest.mark.parametrize("omit_fixed", [False, True])
@pytest.mark.parametrize("keep", [None, [0, 2]])
def test_similarity_frame_matches_bitmap_to_bins(omit_fixed, keep):
    """sums per bin (as the kernel gives them) -> the frame: equal to the pandas restatement, NaN for all-zero bins and
    1.0 for bins whose rows were all dropped"""
    rng = np.random.default_rng(3)
    n, size, step, binlen = 5, 9000, 7, 1000
    names = pd.Index([f"g{i}" for i in range(n)], name="name")
    pos = np.arange(0, size, step)
    bits = (rng.random((len(pos), n)) < 0.7).astype(np.uint8)
    bits[(pos >= 2000) & (pos < 3000)] = 1   # a bin of fixed rows only
    bits[(pos >= 5000) & (pos < 6000)] = 0   # a bin of all-zero rows
    frame = pd.DataFrame(bits, index=pd.RangeIndex(0, size, step), columns=names)
    want = ref.bitmap_to_bins(frame, binlen, omit_fixed, [names[i] for i in keep] if keep else None)
    b, s, e = Genome.similarity_bin_geometry(size, step, binlen)
    cs, kept = _sums(bits, pos // binlen, len(b), omit_fixed, keep)
    got = Genome._similarity_frame(cs, kept, b * binlen, names)
    pd.testing.assert_frame_equal(got, want)
    if omit_fixed:
        assert (got[2000] == 1.0).all()
    if keep is None:
        assert got[5000].isna().all()


class _Rows:
    """stands in for the rows container of one batch"""
    def __init__(self, n):
        self.n = n

    def bin_colsums(self, contigs, starts, ends, step, stride, keep_words, omit_fixed):
        return np.ones((len(starts), self.n), np.uint64), np.ones(len(starts), np.uint64)

    def close(self):
        pass


@pytest.mark.parametrize("step", [1, 100, 300])
def test_batches_are_budgeted_on_full_resolution_rows(step):
    """a rows container holds every bitmap.1 row of its chromosomes even when it reads the low-resolution file: the batch
    budget counts those bytes whatever the step"""
    g = object.__new__(Genome)
    g.name, g.ngenomes, g.nbytes, g.steps = "a", 20, 3, [1, 100]
    g.index = SimpleNamespace(genome_names=pd.Index([f"g{i}" for i in range(20)], name="name"), lowres_step=100)
    g.set_chrs(pd.DataFrame({"size": [50000, 40000, 30000, 0, 20000]},
                            index=pd.Index(["c1", "c2", "c3", "c4", "c5"], name="name")))
    seen = []

    def rows(batch, bstep):
        seen.append((list(batch), bstep))
        return _Rows(20)
    g._rows_from_disk = rows
    g.similarity_budget = 90000 * 3  # c1 + c2 at full resolution: c3 needs a batch of its own
    out = g.kmer_similarity_bins(step=step, bin_size=1000)
    bstep = 100 if step % 100 == 0 else 1
    # (c4 has no rows, so c3 and c5 are not neighbours)
    assert seen == [(["c1", "c2"], bstep), (["c3"], bstep), (["c5"], bstep)]
    assert list(out) == ["c1", "c2", "c3", "c4", "c5"] and out["c4"].shape == (20, 0)


# ---------------------------------------------------------------------------
# preprocessing and genome similarities
# ---------------------------------------------------------------------------
def _frames(seed=0, n=6, nb=40, binlen=1000):
    rng = np.random.default_rng(seed)
    names = pd.Index([f"g{i}" for i in range(n)], name="name")
    out = {}
    for c, nbins in (("chr1", nb), ("chr2", nb // 2 + 3)):
        v = rng.random((n, nbins)) * 0.6 + 0.4
        v[0] = 1.0
        v[:, 3] = np.nan           # an all-zero bin
        v[2, 7] = 1.0
        v[:, 9] = 1.0              # a bin of fixed rows only
        out[c] = pd.DataFrame(v, index=names, columns=pd.Index(np.arange(nbins, dtype=np.int64) * binlen))
    return out


@pytest.mark.parametrize("trm", [3.0, 1.0, -1])
def test_genome_similarities(trm):
    fr = _frames()
    got = it.genome_similarities(list(fr.values()), trm)
    want = ref.similarities(list(fr.values()), trm)
    pd.testing.assert_series_equal(got, want)


@pytest.mark.parametrize("gnm", [None, -1, 0, 0.9])
@pytest.mark.parametrize("sft,ssz", [(None, 5), ("mean", 5), ("median", 3), ("mean", 2)])
@pytest.mark.parametrize("edg", [False, True])
def test_preprocess_matches_restatement(gnm, sft, ssz, edg):
    fr = _frames(1)
    sims = it.genome_similarities(list(fr.values()), 3.0) if gnm else None
    for c, df in fr.items():
        got = it.preprocess(df, sims, gnm, sft, ssz, edg)
        want = ref.preprocess(df, ref.similarities(list(fr.values()), 3.0) if gnm else None, gnm, sft, ssz, edg)
        pd.testing.assert_frame_equal(got, want, check_names=False)
        assert got.index.equals(df.index) and got.columns.equals(df.columns)


def test_gnm_zero_is_no_shift():
    fr = _frames(2)
    sims = it.genome_similarities(list(fr.values()), 3.0)
    df = fr["chr1"]
    pd.testing.assert_frame_equal(it.preprocess(df, None, 0, None, 5, False), df.round(2))
    shifted = it.preprocess(df, sims, 0.9, None, 5, False)
    assert not shifted.equals(df.round(2))


# ---------------------------------------------------------------------------
# thresholds, merged and BED records, through run_call on a stand-in index
# ---------------------------------------------------------------------------
class _Genome:
    def __init__(self, name, frames, tmp):
        self.name, self._frames = name, frames
        self.anchored = frames is not None
        self.chrs = pd.DataFrame({"size": [10 ** 6] * len(frames or {})}, index=pd.Index(list(frames or {}), name="name"))
        d = tmp / name
        d.mkdir(parents=True, exist_ok=True)
        self.chrs_fname = str(d / "chrs.tsv")
        if frames is not None:
            Path(self.chrs_fname).write_text("x")
            (d / "bitmap.1.gz").write_bytes(b"")
        self.calls = []

    def bitmap_gz_fname(self, step):
        return os.path.join(os.path.dirname(self.chrs_fname), f"bitmap.{step}.gz")

    def load_chrs(self):
        pass

    def kmer_similarity_bins(self, chroms=None, step=100, bin_size=1_000_000, omit_fixed=False, keep=None):
        self.calls.append((tuple(chroms), step, bin_size, omit_fixed, tuple(keep) if keep else None))
        return {c: self._frames[c] for c in chroms}


class _Index:
    def __init__(self, genomes):
        self.genomes = genomes

    def __getitem__(self, n):
        return self.genomes[n]

    def close(self):
        pass


GROUPS = {"R1": "REF", "R2": "REF", "C1": "CULT", "C2": "CULT", "W1": "WILD", "W2": "WILD", "X1": "OUT"}


def _scene(tmp_path, seed=4, binlen=1000):
    rng = np.random.default_rng(seed)
    names = pd.Index(list(GROUPS), name="name")
    frames = {}
    for c, nb in (("chr1", 30), ("chr2", 12)):
        v = np.clip(rng.normal(0.9, 0.05, (len(names), nb)), 0, 1)
        v[2] = 1.0                                     # the anchor C1
        v[0:2, 10:16] = rng.uniform(0.3, 0.6, v[0:2, 10:16].shape)  # C1 far from REF here ...
        v[4, 10:16] = 1.0                              # ... and close to W1
        v[0:2, 20:22] = 0.5
        v[5, 20:22] = 1.0
        v[6, 10:22] = 0.3
        v[6, 0:4] = 1.0                                # close to X1 (OUT) only
        v[0:2, 0:4] = 0.75
        v[4:6, 0:4] = 0.85
        v[:, 25 % nb] = np.nan
        frames[c] = pd.DataFrame(v, index=names, columns=pd.Index(np.arange(nb, dtype=np.int64) * binlen))
    tsv = tmp_path / "groups.tsv"
    tsv.write_text("name\tgroup\n" + "".join(f"{n}\t{g}\n" for n, g in GROUPS.items()))
    genomes = {n: _Genome(n, frames if n in ("C1", "R1") else None, tmp_path / "idx") for n in GROUPS}
    return _Index(genomes), frames, str(tsv)


def _args(tmp_path, tsv, extra):
    return it.call_parser().parse_args(["--idx", str(tmp_path / "idx"), "--tsv", tsv, "--out", str(tmp_path / "calls"),
                                     "--bin", "1000"] + extra)


def _restated_beds(frames, anchor, comps, thr, binlen, gnm=None, trm=3.0, sft=None, ssz=5, edg=False, urf=False):
    sims = ref.similarities(list(frames.values()), trm) if gnm else None
    out = {}
    for c, df in frames.items():
        pre = ref.preprocess(df, sims, gnm, sft, ssz, edg)
        merged = None
        for comp in comps:
            calls = (pre.loc[anchor] < thr).astype(int) if urf else ref.calls_3way_or_2way(pre, GROUPS, comp, thr)
            name = comp if urf or comp != "REF" else "REFA"
            out[f"{anchor}_{c}_{name}.bed"] = ref.bed_text(calls, binlen, c, name)
            if len(comps) > 1:
                merged = calls if merged is None else merged + calls
        if merged is not None:
            out[f"{anchor}_{c}_merged.bed"] = ref.bed_text(merged, binlen, c, "merged")
    return out


def _beds(d):
    return {p.name: p.read_text() for p in sorted(Path(d).iterdir())}


@pytest.mark.parametrize("extra,comps,kw", [
    (["--cmp", "WILD", "--thr", "0.2"], ["WILD"], {}),
    (["--cmp", "WILD", "CULT", "OUT", "--thr", "0.2"], ["WILD", "OUT"], {}),
    (["--cmp", "REF", "--thr", "0.7"], ["REF"], {}),
    (["--cmp", "WILD", "--thr", "0.2", "--gnm", "-1", "--sft", "mean", "--ssz", "3"], ["WILD"], dict(gnm=-1, sft="mean", ssz=3)),
    (["--cmp", "WILD", "--thr", "0.1", "--gnm", "0.9", "--trm", "-1", "--sft", "median", "--edg"], ["WILD"],
     dict(gnm=0.9, trm=-1, sft="median", edg=True)),
    (["--cmp", "WILD", "--thr", "0.2", "--gnm", "0"], ["WILD"], {}),
])
def test_calls_match_restatement(tmp_path, extra, comps, kw):
    idx, frames, tsv = _scene(tmp_path)
    a = _args(tmp_path, tsv, ["--anc", "C1"] + extra)
    it.run_call(a, idx=idx, log=lambda *x: None)  # (CULT, the anchor's own group, is dropped from --cmp)
    thr = float(extra[extra.index("--thr") + 1])
    d = tmp_path / "calls" / f"calls_{thr}" / "raw"
    want = _restated_beds(frames, "C1", comps, thr, 1000, **kw)
    assert _beds(d) == want
    if extra[:2] == ["--cmp", "WILD"] and "--gnm" not in extra:
        assert want["C1_chr1_WILD.bed"] == "chr1\t10000\t15999\tWILD_intro\nchr1\t20000\t21999\tWILD_intro\n"
    if "OUT" in extra:
        assert want["C1_chr1_OUT.bed"] == "chr1\t0\t3999\tOUT_intro\n"
        assert want["C1_chr1_merged.bed"] == ("chr1\t0\t3999\tmerged_intro\nchr1\t10000\t15999\tmerged_intro\n"
                                             "chr1\t20000\t21999\tmerged_intro\n")
    # one binning pass per anchor, whatever the thresholds and groups
    assert len(idx["C1"].calls) == 1


def test_urf_and_rmu(tmp_path):
    idx, frames, tsv = _scene(tmp_path)
    a = _args(tmp_path, tsv, ["--anc", "C1", "C2", "--cmp", "REF", "--urf", "--ref", "R1", "--thr", "0.7", "0.8"])
    with pytest.raises(ValueError, match="C2 has no bitmaps"):
        it.run_call(a, idx=idx, log=lambda *x: None)
    a = _args(tmp_path, tsv, ["--anc", "C1", "--cmp", "REF", "--urf", "--ref", "R1", "--thr", "0.7", "0.8"])
    it.run_call(a, idx=idx, log=lambda *x: None)
    for thr in (0.7, 0.8):
        assert _beds(tmp_path / "calls" / f"calls_{thr}" / "raw") == _restated_beds(frames, "C1", ["REF"], thr, 1000, urf=True)
    assert idx["R1"].calls and not idx["C1"].calls  # the reference's view: R1's frames
    # --rmu overrides --urf for the listed anchors: REFA files from the anchor's own frames, with the keep mask
    a = _args(tmp_path, tsv, ["--anc", "C1", "--cmp", "REF", "--urf", "--ref", "R1", "--thr", "0.75", "--rmu", "true",
                              "--ogrp", "WILD", "--rmf"])
    it.run_call(a, idx=idx, log=lambda *x: None)
    assert _beds(tmp_path / "calls" / "calls_0.75" / "raw") == _restated_beds(frames, "C1", ["REF"], 0.75, 1000)
    assert idx["C1"].calls[-1][3:] == (True, ("W1", "W2", "R1"))


def test_layout_and_empty_files(tmp_path):
    idx, frames, tsv = _scene(tmp_path)
    a = _args(tmp_path, tsv, ["--anc", "C1", "--cmp", "WILD", "--thr", "0.99", "--chr", "chr2"])
    it.run_call(a, idx=idx, log=lambda *x: None)
    raw = tmp_path / "calls" / "calls_0.99" / "raw"
    assert sorted(os.listdir(tmp_path / "calls")) == ["calls_0.99"]
    assert sorted(os.listdir(raw)) == ["C1_chr2_WILD.bed"]
    assert (raw / "C1_chr2_WILD.bed").read_text() == ""


def test_anchor_in_compared_group_is_skipped(tmp_path):
    idx, _, tsv = _scene(tmp_path)
    a = _args(tmp_path, tsv, ["--anc", "C1", "--cmp", "CULT", "--thr", "0.2"])
    it.run_call(a, idx=idx, log=lambda *x: None)
    assert not (tmp_path / "calls").exists()


def test_bed_records_join_adjacent_bins_only():
    calls = pd.Series([0, 1, 1, 0, 1, 1, 1], index=[0, 100, 200, 300, 400, 600, 700])
    assert it.bed_records(calls, 100, "c", "W") == [("c", 100, 299, "W_intro"), ("c", 400, 499, "W_intro"),
                                                    ("c", 600, 799, "W_intro")]
    assert ref.bed_text(calls, 100, "c", "W") == "c\t100\t299\tW_intro\nc\t400\t499\tW_intro\nc\t600\t799\tW_intro\n"


# ---------------------------------------------------------------------------
# input errors
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("extra,msg", [
    (["--anc", "C1", "--cmp", "REF", "WILD", "--thr", "0.2"], "REF must be the only comparison group"),
    (["--anc", "C1", "--cmp", "WILD", "--thr", "0.2", "--urf"], "REF must be the only comparison group specified with --cmp"),
    (["--anc", "C1", "--cmp", "WILD", "--thr", "0.2", "--rmu", "C1", "--ogrp", "WILD"], "--ref when using --rmu"),
    (["--anc", "C1", "--cmp", "WILD", "--thr", "0.2", "--rmu", "C1", "--ref", "R1"], "--ogrp when using --rmu"),
    (["--anc", "C1", "--cmp", "WILD", "--thr", "0.2", "--rmu", "W1", "--ref", "R1", "--ogrp", "WILD"], "cannot be in the outgroup"),
    (["--anc", "C1", "--grp", "CULT", "--cmp", "WILD", "--thr", "0.2"], "Cannot use both --anc and --grp"),
    (["--cmp", "WILD", "--thr", "0.2"], "No anchor selected"),
    (["--anc", "C1", "--cmp", "WILD"], "At least one threshold"),
    (["--anc", "C1", "--cmp", "WILD", "--thr", "0.2", "--sft", "max"], "Invalid smoothing filter"),
    (["--anc", "W1", "--cmp", "REF", "--thr", "0.2"], "W1 has no bitmaps"),
])
def test_input_errors(tmp_path, extra, msg):
    idx, _, tsv = _scene(tmp_path)
    with pytest.raises(ValueError, match=msg):
        it.run_call(_args(tmp_path, tsv, extra), idx=idx, log=lambda *x: None)
    assert not (tmp_path / "calls").exists()


def test_group_with_underscore(tmp_path):
    idx, _, _ = _scene(tmp_path)
    tsv = tmp_path / "bad.tsv"
    tsv.write_text("name\tgroup\nC1\tCU_LT\nR1\tREF\n")
    with pytest.raises(ValueError, match="underscores"):
        it.run_call(_args(tmp_path, str(tsv), ["--anc", "C1", "--cmp", "REF", "--thr", "0.2"]), idx=idx)


def test_grp_selects_anchors(tmp_path):
    groups = pd.Series(GROUPS)
    a = it.call_parser().parse_args(["--idx", "i", "--tsv", "t", "--out", "o", "--grp", "CULT", "WILD", "--cmp", "REF",
                                     "--thr", "0.5", "--rmu", "true", "--ogrp", "WILD", "--ref", "R1"])
    with pytest.raises(ValueError, match="cannot be in the outgroup"):
        it.plan(a, groups)
    a.grp = ["CULT"]
    p = it.plan(a, groups)
    assert p["anchors"] == ["C1", "C2"] and p["rmu"] == ["C1", "C2"] and p["keep"] == ["W1", "W2", "R1"]


# ---------------------------------------------------------------------------
# config.yaml and --sweep
# ---------------------------------------------------------------------------
CONFIG = """general:
  output_dir: {out}
  index_dir: {idx}
  tsv: {tsv}
  bin: 125000
  ref: Reference
  threads: 1

calling:
  run: true
  grp: OFFSPRING
  anc: null
  chr: [chr1, chr3]
  cmp: {cmp}
  thr: [0.2, 0.3]
  stp: 100
  gnm: 0.9
  trm: 3
  sft: mean
  ssz: 2
  urf: false
  rmf: true
  rmu: {rmu}
  ogrp: {ogrp}
  edg: false
  vis: {vis}

postprocessing:
  run: {post}
  act: [fgap, rmbn]
  min: 8
  gap: 4
  map: null
  paf: null

scoring:
  run: {score}
  gdt: null
  act: null
  min: null
  gap: null
  thr: null
  cmp: null
  vis: false
"""


def _config(tmp_path, **kw):
    opts = dict(out=tmp_path / "o", idx=tmp_path, tsv=tmp_path / "g.tsv", cmp="[WT]", rmu="null", ogrp="null", vis="false",
                post="false", score="false")
    opts.update(kw)
    p = tmp_path / "c.yaml"
    p.write_text(CONFIG.format(**opts))
    return p


def test_config_to_call_flags(tmp_path):
    argv = it.config_argv(_config(tmp_path))
    a = it.call_parser().parse_args(argv)
    assert Path(a.out) == (tmp_path / "o").resolve() and Path(a.idx) == tmp_path.resolve()
    assert (a.bin, a.stp, a.gnm, a.trm, a.sft, a.ssz, a.rmf, a.urf, a.edg) == (125000, 100, 0.9, 3.0, "mean", 2, True, False, False)
    assert a.grp == ["OFFSPRING"] and a.anc is None and a.chr == ["chr1", "chr3"] and a.cmp == ["WT"]
    assert a.thr == [0.2, 0.3] and a.ref == "Reference" and a.rmu is None
    a = it.call_parser().parse_args(it.config_argv(_config(tmp_path, rmu="true", ogrp="[WT]")))
    assert a.rmu == ["true"] and a.ogrp == ["WT"]
    a = it.call_parser().parse_args(it.config_argv(_config(tmp_path, rmu="[A, B]", ogrp="[WT]")))
    assert a.rmu == ["A", "B"]


def test_sweep_lists(tmp_path):
    a = it.call_parser().parse_args(it.config_argv(_config(tmp_path), sweep=True))
    assert a.thr == [round(0.04 * i, 2) for i in range(18)]
    a = it.call_parser().parse_args(it.config_argv(_config(tmp_path, cmp="[REF]"), sweep=True))
    assert a.thr == [round(0.1 + 0.05 * i, 2) for i in range(18)]
    assert [it.threshold_dir(Path("/x/out"), t).name for t in a.thr][:3] == ["out_0.1", "out_0.15", "out_0.2"]
    assert it.threshold_dir(Path("/x/out/"), 0.0).name == "out_0.0"


@pytest.mark.parametrize("which", ["post", "score"])
def test_config_out_of_scope_steps_fail_first(tmp_path, which):
    with pytest.raises(ValueError, match="not provided"):
        it.run_config(_config(tmp_path, **{which: "true"}))
    assert not (tmp_path / "o").exists()


def test_config_vis_warns(tmp_path):
    with pytest.warns(UserWarning, match="not provided"):
        it.config_argv(_config(tmp_path, vis="true"))


def test_config_missing_file(tmp_path):
    with pytest.raises(ValueError, match="does not exist"):
        it.config_argv(tmp_path / "nope.yaml")


def test_cli_usage(capsys):
    from panagram_amd.__main__ import main
    assert main(["intros"]) == 0
    assert "intros call" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        main(["intros", "call", "--idx", "x"])


def test_product_names_no_test_helper():
    src = open(it.__file__).read()
    assert "intros_ref" not in src and "oracle" not in src
