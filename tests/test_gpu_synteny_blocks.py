"""GPU: pg_synteny_blocks — table, mates, runs and blocks in one call, the runs never leaving HBM — on the planted genomes of
tests/blocks_ref.py against the numpy model of the blocks over the numpy model of the runs, exactly; then
Index.synteny_blocks_tables and `synteny --blocks` on an index written by Index.run()."""
import numpy as np
import pandas as pd
import pytest

from oracle import pyoracle as po
from panagram_amd import synteny
from tests import blocks_ref as br
from tests import synteny_ref as sr

pytestmark = pytest.mark.gpu

K = sr.PLANTED_K
PG_E_INVALID = -1
WIDE = dict(min_run=1, max_gap=1000, max_shift=100)
# per case the parameters that decide it: bridged, and broken where the planted difference passes a bound
PARAMS = {"snps": [WIDE, dict(min_run=1, max_gap=1, max_shift=0)],
          "indel": [WIDE, dict(min_run=1, max_gap=1000, max_shift=br.INS_LEN - 1), dict(min_run=1, max_gap=1000, max_shift=br.DEL_LEN - 1)],
          "inversion": [WIDE],
          "translocation": [WIDE, dict(min_run=1, max_gap=1000, max_shift=300)],
          "stray": [WIDE, dict(min_run=br.STRAY_KMERS + 1, max_gap=1000, max_shift=100)],
          "three_b": [WIDE]}


def _both(ctx, case, k, **params):
    """(synteny_blocks, synteny_segments) of a planted case"""
    from panagram_amd import engine
    a, b = ([sr.ascii_of(c) for c in side] for side in case)
    ssa, ssb = engine.SeqSet.from_host(ctx, a), engine.SeqSet.from_host(ctx, b)
    try:
        return engine.synteny_blocks(ctx, k, ssa, ssb, **params), engine.synteny_segments(ctx, k, ssa, ssb)
    finally:
        ssa.close()
        ssb.close()


@pytest.mark.parametrize("k", [15, 32])
@pytest.mark.parametrize("name", sorted(PARAMS))
def test_synteny_blocks_equal_the_model(ctx, name, k):
    case = br.planted_cases(k)[name]
    runs, mated, lens_b = br.case_runs(case, k)
    extra = []
    if name == "indel":  # the insertion is dA = k, dB = k + 7 and the deletion dA = k + 5, dB = k: past max_gap on ONE genome only
        extra = [dict(min_run=1, max_gap=k + br.INS_LEN - 1, max_shift=100), dict(min_run=1, max_gap=k + br.DEL_LEN - 1, max_shift=100)]
        assert [len(br.blocks(runs, lens_b, **p)) for p in extra] == [2, 3]
    for params in PARAMS[name] + extra:
        want = br.blocks(runs, lens_b, **params)
        got, seg = _both(ctx, case, k, **params)
        have = np.stack(got[:8], axis=1).astype(np.int64)
        assert have.tolist() == want.tolist(), (name, k, params)
        assert got[8].astype(np.int64).tolist() == np.bincount(want[:, 0], minlength=len(case[0]))[:len(case[0])].tolist()
        # nmated and nruns: what synteny_segments returns for the same inputs, which is the model's
        assert got[9] == seg[5] == mated and got[10] == len(seg[0]) == len(runs), (name, k)
    if name == "three_b":  # three contigs of B: the runs lie k apart on both genomes, and no block crosses an edge
        assert len(want) == 3 and len(br.blocks(runs, [sum(lens_b)], **WIDE)) == 1
    if name == "snps":
        assert [len(br.blocks(runs, lens_b, **p)) for p in PARAMS[name]] == [2, len(runs)]


def test_synteny_blocks_capacity_and_timing(ctx):
    from panagram_amd import engine
    case = br.planted_cases(K)["translocation"]
    runs, _, lens_b = br.case_runs(case, K)
    want = br.blocks(runs, lens_b, **WIDE)
    for cap in (0, 1, len(want), len(want) + 3):  # (engine.synteny_blocks calls again when there are more)
        got, _ = _both(ctx, case, K, cap=cap, **WIDE)
        assert np.stack(got[:8], axis=1).astype(np.int64).tolist() == want.tolist(), cap
    ms = engine.synteny_blocks_last_timing()
    assert list(ms) == ["insert_a_ms", "insert_b_ms", "mates_ms", "runs_count_ms", "runs_emit_ms", "blocks_count_ms", "blocks_emit_ms"]
    assert all(v > 0 for v in ms.values()), ms


def test_synteny_blocks_invalid_arguments_and_empty_sides(ctx):
    from panagram_amd import engine
    ss = engine.SeqSet.from_host(ctx, [sr.ascii_of(sr.random_codes(200, 5))])
    short = engine.SeqSet.from_host(ctx, [b"ACGT"])
    try:
        for kw in (dict(min_run=0), dict(max_gap=0), dict(max_gap=1 << 31), dict(max_shift=1 << 31)):
            with pytest.raises(engine.PanagramHipError) as ei:
                engine.synteny_blocks(ctx, K, ss, ss, **{**WIDE, **kw})
            assert ei.value.code == PG_E_INVALID, kw
        for k in (0, 33):
            with pytest.raises(engine.PanagramHipError) as ei:
                engine.synteny_blocks(ctx, k, ss, ss)
            assert ei.value.code == PG_E_INVALID
        got = engine.synteny_blocks(ctx, K, ss, short)  # no k-mer on one side
        assert all(len(a) == 0 for a in got[:8]) and got[8].tolist() == [0] and got[9:] == (0, 0)
        got = engine.synteny_blocks(ctx, K, ss, ss)     # a genome against itself: one block of one run
        n = 200 - K + 1
        assert np.stack(got[:8], axis=1).tolist() == [[0, 0, n, 0, (n - 1) << 1, n, 1, 0]] and got[9:] == (n, 1)
    finally:
        ss.close()
        short.close()


# ---------------------------------------------------------------------------
# Index.synteny_blocks_tables and the subcommand
# ---------------------------------------------------------------------------
CHROMS = ["chr1", "chr2"]


def _genomes():
    x, y = sr.planted_contigs()
    xs, ys = sr.plant_snps(x, br.SNPS[0]), sr.plant_snps(y, br.SNPS[1])
    return [[sr.ascii_of(c) for c in g] for g in ([x, y], sr.planted_rearranged(xs, ys))]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    from panagram_amd import index as pidx
    tmp = tmp_path_factory.mktemp("synteny_blocks")
    lines = ["name\tfasta"]
    for i, contigs in enumerate(_genomes()):
        fa = tmp / f"g{i}.fa"
        fa.write_bytes(po.fasta_text(CHROMS, contigs))
        lines.append(f"g{i}\t{fa}")
    (tmp / "samples.tsv").write_text("\n".join(lines) + "\n")
    out = str(tmp / "idx")
    pidx.Index(str(tmp / "samples.tsv"), prefix=out, k=K, anchor_genomes=["g0"], lowres_step=100).run()
    return out


def _want(k=K, min_len=1, **params):
    a, b = _genomes()
    runs, mated = sr.segments(a, b, k)
    lens_b = [len(c) for c in b]
    return br.block_rows(br.blocks(runs, lens_b, **params), k, CHROMS, lens_b, CHROMS, min_len), mated, len(runs)


def _rows(frame):
    assert list(frame.columns) == synteny.BLOCK_COLUMNS
    return [tuple(r) for r in frame.values.tolist()]


def test_index_synteny_blocks_tables_equal_the_model(built):
    from panagram_amd import index as pidx
    idx = pidx.Index(built, mode="r")
    try:
        want, mated, nruns = _want(**WIDE)
        # the substitutions are bridged, the rearrangements are not: chr1's head, the moved block on chr2, chr1's tail, ...
        assert len(want) < nruns and [r[:7] for r in want[:3]] == [("chr1", 0, 200, "chr1", 0, 200, "+"), ("chr1", 200, 500, "chr2", 300, 600, "+"),
                                                                   ("chr1", 500, 900, "chr1", 200, 600, "+")]
        assert [r[8] for r in want[:3]] == [2, 2, 2] and ("chr2", 100, 140, "chr2", 100, 140, "-", 40 - K + 1, 1, 0) in want
        blk, summary, totals, lens = idx.synteny_blocks_tables("g0", "g1")
        assert _rows(blk) == want
        assert summary.iloc[-1].tolist() == ["*", "*", "*", len(want), mated] and summary.equals(synteny.summary_frame(blk))
        assert totals.equals(idx.synteny_tables("g0", "g1")[2])
        assert lens == ({"chr1": 900, "chr2": 700}, {"chr1": 600, "chr2": 1000})
        narrow = dict(min_run=20, max_gap=40, max_shift=0)
        assert _rows(idx.synteny_blocks_tables("g0", "g1", k=21, min_len=50, **narrow)[0]) == _want(21, 50, **narrow)[0]
        assert _rows(idx.synteny_blocks_tables("g0", "g1", chroms_a=["chr2"])[0]) == [r for r in want if r[0] == "chr2"]
        for bad in (dict(min_run=0), dict(max_gap=0), dict(max_gap=1 << 31), dict(max_shift=-1), dict(k=33), dict(chroms_b=["chr9"])):
            with pytest.raises(ValueError):
                idx.synteny_blocks_tables("g0", "g1", **bad)
    finally:
        idx.close()


def test_synteny_blocks_subcommand(built, tmp_path, capsys):
    from panagram_amd.__main__ import main
    want, mated, _ = _want(**WIDE)
    out, summ = tmp_path / "blocks.tsv", tmp_path / "summary.tsv"
    assert main(["synteny", built, "g0", "g1", "--blocks", "-o", str(out), "--summary", str(summ)]) == 0
    got = pd.read_csv(out, sep="\t", header=None, names=synteny.BLOCK_COLUMNS)
    assert _rows(got) == want
    s = pd.read_csv(summ, sep="\t", comment="#")
    assert list(s.columns) == synteny.SUMMARY_COLUMNS and s.iloc[-1].tolist() == ["*", "*", "*", len(want), mated]
    assert s.values.tolist() == synteny.summary_frame(got).values.tolist()
    # the link flags and --min-len (on blocks: their k-mers), to stdout
    capsys.readouterr()
    flags = dict(min_run=20, max_gap=K, max_shift=0)  # (a substitution's link is K + 1 wide: not bridged any more)
    assert main(["synteny", built, "g0", "g1", "--blocks", "--min-run", "20", "--max-gap", str(K), "--max-shift", "0", "--min-len", "50"]) == 0
    lines = [tuple(int(v) if v.isdigit() else v for v in ln.split("\t")) for ln in capsys.readouterr().out.splitlines()]
    assert lines == _want(K, 50, **flags)[0] and lines != [r for r in want if r[7] >= 50]
    # PAF: the same blocks, query A and target B
    assert main(["synteny", built, "g0", "g1", "--blocks", "--paf"]) == 0
    paf = capsys.readouterr().out.splitlines()
    la, lb = {"chr1": 900, "chr2": 700}, {"chr1": 600, "chr2": 1000}
    assert paf == ["\t".join(str(v) for v in (r[0], la[r[0]], r[1], r[2], r[6], r[3], lb[r[3]], r[4], r[5], r[7], max(r[2] - r[1], r[5] - r[4]), 255,
                                              f"rn:i:{r[8]}", f"sh:i:{r[9]}")) for r in want]
    assert paf[1] == f"chr1\t900\t200\t500\t+\tchr2\t1000\t300\t600\t{300 - K + 1 - K}\t300\t255\trn:i:2\tsh:i:0"
    # without --blocks the output is the runs', and the block flags are refused before the index is opened
    assert main(["synteny", built, "g0", "g1"]) == 0
    assert len(capsys.readouterr().out.splitlines()) == _want(**WIDE)[2]
    for flags in (["--paf"], ["--min-run", "2"], ["--max-gap", "10"], ["--max-shift", "1"]):
        with pytest.raises(SystemExit) as ei:
            main(["synteny", "/nonexistent", "g0", "g1"] + flags)
        assert ei.value.code == 2 and "need --blocks" in capsys.readouterr().err
    for flags in (["--min-run", "0"], ["--max-gap", "0"], ["--max-shift", "-1"]):
        with pytest.raises(SystemExit) as ei:
            main(["synteny", built, "g0", "g1", "--blocks"] + flags)
        assert ei.value.code == 2 and flags[0][2:].replace("-", "_") in capsys.readouterr().err
