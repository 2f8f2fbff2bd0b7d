"""GPU: pg_synteny_variants — table, mates, runs, blocks and variants in one call, nothing but the variants leaving HBM — on the
planted genomes of tests/variants_ref.py against the numpy model of the variants over the numpy model of the runs, exactly; the
invariant on the GPU's own records; then Index.synteny_variants_tables and `synteny --variants [--vcf]` on an index written by
Index.run()."""
import numpy as np
import pandas as pd
import pytest

from oracle import pyoracle as po
from panagram_amd import synteny
from tests import blocks_ref as br
from tests import synteny_ref as sr
from tests import variants_ref as vr

pytestmark = pytest.mark.gpu

K = sr.PLANTED_K
PG_E_INVALID = -1
WIDE = dict(min_run=1, max_gap=1000, max_shift=100)
CASES = sorted(vr.planted_cases(K))


@pytest.fixture(scope="module")
def cases():
    return vr.planted_cases(K)


class _Sides:
    def __init__(self, ctx, case):
        from panagram_amd import engine
        self.a, self.b = engine.SeqSet.from_host(ctx, case[0]), engine.SeqSet.from_host(ctx, case[1])

    def __enter__(self):
        return self.a, self.b

    def __exit__(self, *exc):
        self.a.close()
        self.b.close()


def _records(got):
    return np.stack(got[:7], axis=1).astype(np.int64).tolist(), np.stack(got[7:9], axis=1).tolist()


@pytest.mark.parametrize("name", CASES)
def test_synteny_variants_equal_the_model_and_run_variants(ctx, cases, name):
    from panagram_amd import engine
    case = cases[name]
    a, b, params, _ = case
    runs, mated = vr.case_runs(case, K)
    m = vr.variants(runs, a, b, K, **params)
    with _Sides(ctx, case) as (ssa, ssb):
        got = engine.synteny_variants(ctx, K, ssa, ssb, **params)
        rc, rs, re_, rm, _, nmated = engine.synteny_segments(ctx, K, ssa, ssb)
        fed = engine.run_variants(ctx, K, ssa, ssb, rc, rs, re_, rm, **params)
        blk = engine.synteny_blocks(ctx, K, ssa, ssb, **params)
        frame = synteny.variant_frame(*got[:9], [f"a{i}" for i in range(len(a))], [len(c) for c in b], [f"b{i}" for i in range(len(b))], ssa, ssb)
    print(name, "classes", got[9].tolist(), m["classes"], "links", got[10], m["links"], "records", len(got[0]))
    # the model on the model's runs: order and every field
    assert _records(got) == (m["records"].tolist(), m["words"].tolist())
    assert got[9].astype(np.int64).tolist() == m["classes"] and got[10] == m["links"] == int(got[9].sum())
    assert got[11:] == (mated, len(runs), len(m["blocks"])) and nmated == mated
    # run_variants fed with synteny_segments' runs
    assert np.stack([rc, rs, re_, rm], axis=1).astype(np.int64).tolist() == runs.tolist()
    assert all(np.array_equal(x, y) for x, y in zip(got[:10], fed[:10])) and fed[10] == got[10]
    # every link of every block, no other: links = the sum of (runs - 1) over synteny_blocks' blocks
    assert got[10] == int((blk[6].astype(np.int64) - 1).sum()) and len(blk[0]) == got[13]
    # the invariant on the GPU's records, every block, alleles beyond 32 bases through variant_frame
    assert [(r.ref.encode(), r.alt.encode()) for r in frame.itertuples()] == m["alleles"]
    for c, s, e, mf, ml in np.stack(blk[:5], axis=1).astype(np.int64).tolist():
        have = synteny.apply_variants(vr.norm(a[c]), frame, s, e + K - 1, chrom=f"a{c}")
        assert have == vr.block_b_range([c, s, e, mf, ml, None], b, K), (name, c, s, e)


def test_synteny_variants_at_the_edges_of_contigs(ctx, cases):
    """a strand-1 allele inside the first 32 bases of B's first contig — the window that would begin before base 0 — and a
    strand-0 allele inside the last 32 bases of both sides' last contig"""
    from panagram_amd import engine
    for name, strand in (("b_start", 1), ("a_end", 0)):
        a, b, params, want = cases[name]
        with _Sides(ctx, cases[name]) as (ssa, ssb):
            got = engine.synteny_variants(ctx, K, ssa, ssb, **params)
            frame = synteny.variant_frame(*got[:9], [str(i) for i in range(len(a))], [len(c) for c in b], [str(i) for i in range(len(b))], ssa, ssb)
        assert [(r.posA, r.ref.encode(), r.alt.encode(), r.strand) for r in frame.itertuples()] == \
               [(q, vr.norm(a[c])[q:q + n], alt, "+-"[st]) for c, q, cls, n, alt, st in want]
        last = frame.iloc[-1]
        if strand:
            assert last.chrB == "0" and last.posB + last.altLen <= 32 and last.strand == "-"
        else:
            assert last.chrB == str(len(b) - 1) and len(b[-1]) - last.posB <= 32 and len(a[-1]) - last.posA <= 32


def test_synteny_variants_capacity_and_timing(ctx, cases):
    from panagram_amd import engine
    case = cases["inverted"]
    a, b, params, _ = case
    m = vr.variants(vr.case_runs(case, K)[0], a, b, K, **params)
    total = len(m["records"])
    assert total == 3
    with _Sides(ctx, case) as (ssa, ssb):
        for cap in (0, total - 1, total, total + 3):  # (engine.synteny_variants calls again when there are more)
            got = engine.synteny_variants(ctx, K, ssa, ssb, cap=cap, **params)
            assert _records(got) == (m["records"].tolist(), m["words"].tolist()), cap
        ms = engine.synteny_variants_last_timing()
        # the protocol itself: nothing is written when the arrays are too short
        import ctypes as C
        arrs = engine._variant_arrays(total - 1)
        cls, counts = np.zeros(6, np.uint64), [C.c_uint64() for _ in range(5)]
        rc = ctx._lib.pg_synteny_variants(ctx._h, K, ssa._h, ssb._h, 1, 1000, 100, total - 1, *[engine._ptr(x) for x in arrs], engine._ptr(cls),
                                          *[C.byref(x) for x in counts])
        assert rc == 0 and counts[1].value == total and counts[0].value == m["links"] and cls.astype(np.int64).tolist() == m["classes"]
        assert all((x == 0xFFFFFFFF).all() for x in arrs[:7]) and all((x == (1 << 64) - 1).all() for x in arrs[7:])
        short = engine.synteny_variants_last_timing()
    assert list(ms) == ["insert_a_ms", "insert_b_ms", "mates_ms", "runs_count_ms", "runs_emit_ms", "blocks_count_ms", "blocks_emit_ms",
                        "variants_count_ms", "variants_emit_ms"]
    assert ms["blocks_emit_ms"] == 0 and all(v > 0 for n, v in ms.items() if n != "blocks_emit_ms"), ms  # (the blocks are not emitted)
    assert short["variants_count_ms"] > 0 and short["variants_emit_ms"] == 0, short


def test_synteny_variants_invalid_arguments_and_empty_sides(ctx):
    from panagram_amd import engine
    ss = engine.SeqSet.from_host(ctx, [sr.ascii_of(sr.random_codes(200, 5))])
    short = engine.SeqSet.from_host(ctx, [b"ACGT"])
    try:
        for kw in (dict(min_run=0), dict(max_gap=0), dict(max_gap=vr.MAX_GAP + 1), dict(max_gap=1 << 31), dict(max_shift=1 << 31)):
            with pytest.raises(engine.PanagramHipError) as ei:
                engine.synteny_variants(ctx, K, ss, ss, **{**WIDE, **kw})
            assert ei.value.code == PG_E_INVALID, kw
        for k in (0, 33):
            with pytest.raises(engine.PanagramHipError) as ei:
                engine.synteny_variants(ctx, k, ss, ss)
            assert ei.value.code == PG_E_INVALID
        got = engine.synteny_variants(ctx, K, ss, short)  # no k-mer on one side
        assert all(len(x) == 0 for x in got[:9]) and got[9].tolist() == [0] * 6 and got[10:] == (0, 0, 0, 0)
        got = engine.synteny_variants(ctx, K, ss, ss, max_gap=vr.MAX_GAP)  # a genome against itself: one block of one run, no link
        assert all(len(x) == 0 for x in got[:9]) and got[10:] == (0, 200 - K + 1, 1, 1)
    finally:
        ss.close()
        short.close()


# ---------------------------------------------------------------------------
# Index.synteny_variants_tables and the subcommand
# ---------------------------------------------------------------------------
CHROMS = ["chr1", "chr2"]
SNPS1 = (100, 800)


def _genomes():
    """A: the insertion-and-deletion contig of tests/blocks_ref.py and a second contig; B: the insertion, the deletion and two
    substitutions in the first, two substitutions in the second"""
    codes = br.planted_cases(K)
    x = sr.ascii_of(codes["indel"][0][0])
    xb = sr.ascii_of(codes["indel"][1][0])
    y = sr.ascii_of(sr.planted_contigs()[1])
    edits1 = [(q, 1, bytes([vr._other(x[q])])) for q in SNPS1] + [(br.INS_AT, 0, xb[br.INS_AT:br.INS_AT + br.INS_LEN]), (br.DEL_AT, br.DEL_LEN, b"")]
    edits2 = [(q, 1, bytes([vr._other(y[q])])) for q in br.SNPS[1]]
    return [x, y], [vr.plant(x, edits1), vr.plant(y, edits2)], [sorted(edits1), sorted(edits2)]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    from panagram_amd import index as pidx
    tmp = tmp_path_factory.mktemp("synteny_variants")
    lines = ["name\tfasta"]
    for i, contigs in enumerate(_genomes()[:2]):
        fa = tmp / f"g{i}.fa"
        fa.write_bytes(po.fasta_text(CHROMS, contigs))
        lines.append(f"g{i}\t{fa}")
    (tmp / "samples.tsv").write_text("\n".join(lines) + "\n")
    out = str(tmp / "idx")
    pidx.Index(str(tmp / "samples.tsv"), prefix=out, k=K, anchor_genomes=["g0"], lowres_step=100).run()
    return out


def _want_rows():
    """the planted differences as table rows, written from the edits: (chrA, posA, refLen, class, ref, alt)"""
    a, b, edits = _genomes()
    rows = []
    for chrom, seq, es in zip(CHROMS, a, edits):
        for q, n, alt in es:
            cls = "snp" if n == len(alt) == 1 else ("ins" if n == 0 else "del")
            rows.append((chrom, q, n, cls, seq[q:q + n].decode(), alt.decode()))
    return rows


def test_index_synteny_variants_tables(built):
    from panagram_amd import index as pidx
    a, b, _ = _genomes()
    idx = pidx.Index(built, mode="r")
    try:
        var, summary, totals, lens = idx.synteny_variants_tables("g0", "g1")
        assert list(var.columns) == synteny.VARIANT_COLUMNS
        assert [(r.chrA, r.posA, r.refLen, r[7], r.ref, r.alt) for r in var.itertuples(index=False)] == _want_rows()
        assert var["strand"].tolist() == ["+"] * 6 and var["chrB"].tolist() == ["chr1"] * 4 + ["chr2"] * 2
        assert var["posB"].tolist() == [100, 300, 607, 802, 50, 400]
        assert summary.values.tolist() == [["snp", 4, 4, 4], ["mnp", 0, 0, 0], ["ins", 1, 0, 7], ["del", 1, 5, 0], ["complex", 0, 0, 0],
                                           ["same", 0, 0, 0], ["links", 6, 9, 11]]
        assert totals.equals(idx.synteny_blocks_tables("g0", "g1")[2])
        assert lens == ({"chr1": 900, "chr2": 700}, {"chr1": 902, "chr2": 700})
        # B as A's chromosomes with the variants carried out
        for chrom, sa, sb in zip(CHROMS, a, b):
            assert synteny.apply_variants(sa, var, chrom=chrom) == sb
        assert [r[0] for r in idx.synteny_variants_tables("g0", "g1", chroms_a=["chr2"])[0].values.tolist()] == ["chr2"] * 2
        for bad in (dict(min_run=0), dict(max_gap=0), dict(max_gap=65537), dict(max_shift=-1), dict(k=33), dict(chroms_b=["chr9"])):
            with pytest.raises(ValueError):
                idx.synteny_variants_tables("g0", "g1", **bad)
    finally:
        idx.close()


def test_synteny_variants_subcommand(built, tmp_path, capsys):
    from panagram_amd.__main__ import main
    a, b, _ = _genomes()
    want = _want_rows()
    out, summ = tmp_path / "variants.tsv", tmp_path / "summary.tsv"
    assert main(["synteny", built, "g0", "g1", "--variants", "-o", str(out), "--summary", str(summ)]) == 0
    got = pd.read_csv(out, sep="\t", header=None, names=synteny.VARIANT_COLUMNS, keep_default_na=False)
    assert [(r.chrA, r.posA, r.refLen, r[7], r.ref, r.alt) for r in got.itertuples(index=False)] == \
           [(c, q, n, cls, ref or "-", alt or "-") for c, q, n, cls, ref, alt in want]
    s = pd.read_csv(summ, sep="\t", comment="#")
    assert list(s.columns) == synteny.VARIANT_SUMMARY_COLUMNS
    by = {r[0]: r[1:] for r in s.values.tolist()}
    assert by["snp"] == [4, 4, 4] and by["ins"] == [1, 0, 7] and by["del"] == [1, 5, 0] and by["same"] == [0, 0, 0]
    assert by["links"][0] == sum(by[c][0] for c in synteny.VARIANT_CLASSES) == 6                      # the summary adds up
    assert by["links"][1:] == [sum(by[c][i] for c in synteny.VARIANT_CLASSES) for i in (1, 2)] == [9, 11]
    assert open(summ).readline().startswith("# side")
    # VCF to stdout: parsed line by line
    capsys.readouterr()
    assert main(["synteny", built, "g0", "g1", "--variants", "--vcf"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == "##fileformat=VCFv4.2" and lines[1:3] == ["##contig=<ID=chr1,length=900>", "##contig=<ID=chr2,length=700>"]
    head = [ln for ln in lines if ln.startswith("#")]
    assert head[-1].split("\t") == ["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT", "g1"]
    assert all(ln.startswith("##") for ln in head[:-1]) and lines[:len(head)] == head
    declared = {ln.split("ID=")[1].split(",")[0] for ln in head if ln.startswith("##INFO")}
    body = [ln.split("\t") for ln in lines[len(head):]]
    assert len(body) == len(want)
    for f, (chrom, q, n, cls, ref, alt) in zip(body, want):
        assert len(f) == 10 and f[0] == chrom and f[2] == "." and f[5:7] == [".", "PASS"] and f[8:] == ["GT", "1"]
        info = dict(kv.split("=") for kv in f[7].split(";"))
        assert set(info) == declared and info["CLASS"] == cls and info["STRAND"] == "+" and info["BCHR"] == chrom
        seq = a[CHROMS.index(chrom)]
        if cls == "snp":
            assert (int(f[1]), f[3], f[4]) == (q + 1, ref, alt) and info["MISM"] == "1"
        else:  # behind the anchor base, at its 1-based position
            anchor = chr(seq[q - 1])
            assert (int(f[1]), f[3], f[4]) == (q, anchor + ref, anchor + alt)
        assert seq[int(f[1]) - 1:int(f[1]) - 1 + len(f[3])].decode() == f[3]                             # REF is A's own text
        sb = b[CHROMS.index(chrom)]
        lo = int(info["BPOS"]) - 1
        assert sb[lo:lo + len(alt)].decode() == alt
    # the link flags reach the kernel: past max_shift the insertion and the deletion break their blocks and are not links
    assert main(["synteny", built, "g0", "g1", "--variants", "--max-shift", "0"]) == 0
    rows = [ln.split("\t") for ln in capsys.readouterr().out.splitlines()]
    assert [r[7] for r in rows] == ["snp"] * 4
    for flags in (["--max-gap", "65537"], ["--min-run", "0"], ["--max-shift", "-1"]):
        with pytest.raises(SystemExit) as ei:
            main(["synteny", built, "g0", "g1", "--variants"] + flags)
        assert ei.value.code == 2 and flags[0][2:].replace("-", "_") in capsys.readouterr().err
