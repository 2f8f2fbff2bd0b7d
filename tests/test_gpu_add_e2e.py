"""GPU: `add` end to end on the golden fixtures, whose trees the reference binary made: an index of the first N_old samples,
then ``Index.add`` of the rest, gives the files the reference wrote for ALL samples — and the tree a from-scratch
``Index.run()`` of all samples gives.

The rule two trees are compared under (that of tests/test_gpu_index_e2e.py's ``_same_index_payload``, restated): the
decompressed bitmaps and every table byte for byte — the compressed bytes and the .gzi follow the BGZF block boundaries,
which may differ — with each .gzi addressing its own payload; logs/ (timings) and config.yaml (it names the samples table
the index was made from) are not part of the index's payload, and kmc/opdef{i}.txt are compared with the tree's own path
taken out."""
import gzip
import os

import numpy as np
import pandas as pd
import pytest

from oracle import pyoracle as po
from tests import helpers as H

pytestmark = pytest.mark.gpu


def _same_index_payload(one, many):
    from panagram_amd import index as pidx
    seen = 0
    for dirpath, _, files in os.walk(one):
        if os.path.basename(dirpath) == "logs":
            continue
        for f in files:
            a = os.path.join(dirpath, f)
            b = os.path.join(many, os.path.relpath(a, one))
            if f.endswith(".gzi") or f == "config.yaml":
                continue
            seen += 1
            if f.endswith(".gz"):
                raw = gzip.open(b, "rb").read()
                assert gzip.open(a, "rb").read() == raw, a
                if os.path.exists(b + "i"):  # (the bitmaps; the annotation tracks carry a .csi)
                    blocks = pidx.load_bgz_blocks(b + "i")
                    for start in (0, len(raw) // 3, max(0, len(raw) - 5)):
                        assert pidx.bgzf_read(b, blocks, start, 5) == raw[start:start + 5]
            elif f.startswith("opdef"):  # (kmc/opdef{i}.txt name the databases by their path inside the tree)
                assert open(a).read().replace(str(one), "@") == open(b).read().replace(str(many), "@"), a
            else:
                assert open(a, "rb").read() == open(b, "rb").read(), a
    assert seen
    files = lambda root: sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs
                                if os.path.basename(d) != "logs")
    assert files(one) == files(many)  # nothing extra either way (no staging directory left)


def _tree_bytes(root):
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read()
            for d, _, fs in os.walk(root) for f in fs}


def _tables(tmp_path, fx, cuts, gffs=None):
    """the case's FASTA files and one samples table per range of samples cut at ``cuts`` (name, fasta, gff, anchor)"""
    n = int(fx["ngenomes"])
    anchors = {int(g) for g in fx["anchors"]}
    gffs = gffs or {}
    rows = []
    for g in range(n):
        fa = tmp_path / f"g{g}.fa"
        fa.write_bytes(fx[f"fasta_{g}"].tobytes())
        rows.append((f"g{g}", str(fa), gffs.get(g, ""), g in anchors))
    out = []
    for i, (lo, hi) in enumerate(zip([0] + list(cuts), list(cuts) + [n])):
        p = tmp_path / f"samples_{i}.tsv"
        pd.DataFrame(rows[lo:hi], columns=["name", "fasta", "gff", "anchor"]).to_csv(p, sep="\t", index=False)
        out.append(str(p))
    allp = tmp_path / "samples_all.tsv"
    pd.DataFrame(rows, columns=["name", "fasta", "gff", "anchor"]).to_csv(allp, sep="\t", index=False)
    return out, str(allp)


def _check_golden(out, fx):
    n, k = int(fx["ngenomes"]), int(fx["k"])
    dbs = H.case_dbs(fx)
    for g in fx["anchors"]:
        adir = out / "anchor" / f"g{g}"
        for step in (1, 100):
            assert gzip.open(adir / f"bitmap.{step}.gz", "rb").read() == fx[f"a{g}_bitmap{step}"].tobytes(), (g, step)
            gzi = np.fromfile(adir / f"bitmap.{step}.gzi", "<u8")
            assert gzi[0] == np.frombuffer(fx[f"a{g}_gzi{step}"].tobytes(), "<u8")[0]
        assert (adir / "bitsum.bins.tsv").read_bytes() == fx[f"a{g}_bitsum.bins.tsv"].tobytes()
        assert (adir / "chrs.tsv").read_bytes() == fx[f"a{g}_chrs.tsv"].tobytes()
        ora = po.anchor_fasta(dbs, fx[f"fasta_{g}"].tobytes(), k, n)
        tp = pd.read_csv(adir / "total_paircounts.csv", index_col="name", float_precision="round_trip")
        assert list(tp.index) == [f"g{i}" for i in range(n)]
        assert np.array_equal(tp["count"].to_numpy(), ora["colsums"])
        assert np.allclose(tp["frac"].to_numpy(), ora["colsums"] / ora["colsums"][g], rtol=0, atol=0)


def _check_queries(out, fx):
    """the read side on the added-to tree: query == unpackbits of the golden payload"""
    from panagram_amd import index as pidx
    n, k = int(fx["ngenomes"]), int(fx["k"])
    ridx = pidx.Index(str(out), mode="r")
    assert list(ridx.genome_names) == [f"g{i}" for i in range(n)]
    g = int(fx["anchors"][0])
    nb = (n + 7) // 8
    rows = np.frombuffer(fx[f"a{g}_bitmap1"].tobytes(), np.uint8).reshape(-1, nb)
    bits = np.unpackbits(rows, axis=1, bitorder="little")[:, :n]
    off = 0
    for nm, seq in po.parse_fasta_cpp(fx[f"fasta_{g}"].tobytes()):
        nk = len(seq) - k + 1
        df = ridx.query_bitmap(f"g{g}", nm, 100, min(nk, 700))
        assert list(df.columns) == [f"g{i}" for i in range(n)]
        assert np.array_equal(df.to_numpy(), bits[off + 100: off + min(nk, 700)])
        assert np.array_equal(ridx.query_bitmap(f"g{g}", nm, 0, nk, 100).to_numpy(), bits[off: off + nk: 100])
        off += nk


def _fresh(tmp_path, allp, k, **kw):
    from panagram_amd import index as pidx
    fresh = tmp_path / "fresh"
    pidx.Index(allp, prefix=str(fresh), k=k, **kw).run()
    return fresh


# (n40_k31 as 29 + 11: two probe tables, of 8 and of 3 new samples — two column blocks of 8, the second one short)
CASES = [("n2_k21", 1), ("n9_k21", 8), ("n40_k31", 38), ("n65_k21", 64), ("n65_k21", 57), ("n40_k31", 29)]


@pytest.mark.parametrize("name, n_old", CASES, ids=[f"{c}_{n}" for c, n in CASES])
def test_add_gives_the_reference_tree_and_the_fresh_one(name, n_old, tmp_path):
    from panagram_amd import index as pidx
    fx = H.load_case(name)
    k = int(fx["k"])
    (old_tsv, new_tsv), allp = _tables(tmp_path, fx, [n_old])
    out = tmp_path / "idx"
    pidx.Index(old_tsv, prefix=str(out), k=k).run()
    idx = pidx.Index(str(out), mode="w")
    lines = idx.add(new_tsv)
    idx.close()
    anchors = [int(g) for g in fx["anchors"]]
    assert lines == [f"rewrote anchor g{g}: {n_old} -> {int(fx['ngenomes'])} samples" for g in anchors if g < n_old] + \
                    [f"added anchor g{g}: {int(fx['ngenomes'])} samples" for g in anchors if g >= n_old]
    _check_golden(out, fx)
    _check_queries(out, fx)
    _same_index_payload(str(_fresh(tmp_path, allp, k)), str(out))


def test_two_adds_equal_one(tmp_path):
    from panagram_amd import index as pidx
    fx = H.load_case("n9_k21")
    k = int(fx["k"])
    (t0, t1, t2), allp = _tables(tmp_path, fx, [7, 8])
    out = tmp_path / "idx"
    pidx.Index(t0, prefix=str(out), k=k).run()
    for t in (t1, t2):
        idx = pidx.Index(str(out), mode="w")
        idx.add(t)
        idx.close()
    _check_golden(out, fx)
    _same_index_payload(str(_fresh(tmp_path, allp, k)), str(out))


def test_add_reexports_the_kmc_databases(tmp_path):
    """with kmc/bitvec* in the index the add never loads them, re-exports them for all samples, and a later table from them is
    the new one"""
    from panagram_amd import index as pidx
    fx = H.load_case("n9_k21")
    k = int(fx["k"])
    (old_tsv, new_tsv), allp = _tables(tmp_path, fx, [8])
    out = tmp_path / "idx"
    pidx.Index(old_tsv, prefix=str(out), k=k, export_kmc=True).run()
    assert (out / "kmc" / "bitvec0.kmc_pre").exists()
    idx = pidx.Index(str(out), mode="w")
    idx.kmc.use_existing = True
    idx.add(new_tsv)
    idx.close()
    _check_golden(out, fx)
    for i, (fk, fm) in enumerate(H.case_dbs(fx)):
        db = po.read_kmc1(str(out / "kmc" / f"bitvec{i}"))
        assert np.array_equal(db["keys"], fk) and np.array_equal(db["counters"], fm)
    assert "g8" in (out / "kmc" / "opdef0.txt").read_text() and ".add_staging" not in (out / "kmc" / "opdef0.txt").read_text()
    idx2 = pidx.Index(str(out), mode="w")
    idx2.kmc.use_existing = True
    a0 = f"g{int(fx['anchors'][0])}"
    idx2.genomes[a0].run_anchor(idx2.build_table())
    idx2.close()
    assert gzip.open(out / "anchor" / a0 / "bitmap.1.gz", "rb").read() == fx[f"a{int(fx['anchors'][0])}_bitmap1"].tobytes()
    _same_index_payload(str(_fresh(tmp_path, allp, k, export_kmc=True)), str(out))


def _gff_for(fx, g, tmp_path):
    recs = po.parse_fasta_cpp(fx[f"fasta_{g}"].tobytes())
    lines = []
    for nm, seq in recs:
        for s, e in ((10, 400), (350, 900), (len(seq) // 2, len(seq) // 2 + 1000), (5, 5 + len(seq))):  # the last: out of bounds
            lines.append(f"{nm}\tsrc\tgene\t{s}\t{e}\t.\t+\t.\tID=x;Name=x\n")
    p = tmp_path / f"g{g}.gff"
    p.write_text("".join(lines))
    return str(p)


def test_annotated_anchor_and_derived_files(tmp_path):
    """an annotated old anchor gets the bitsum.genes.tsv and gene_count a fresh index has; genome_dist.tsv, present
    before, is refreshed, kmer_shared.tsv and the umaps, absent before, stay absent"""
    from panagram_amd import index as pidx
    fx = H.load_case("n9_k21")
    k = int(fx["k"])
    gffs = {0: _gff_for(fx, 0, tmp_path)}
    (old_tsv, new_tsv), allp = _tables(tmp_path, fx, [8], gffs)
    out = tmp_path / "idx"
    pidx.Index(old_tsv, prefix=str(out), k=k, genome_dist=True).run()
    before = (out / "genome_dist.tsv").read_bytes()
    assert (out / "anchor" / "g0" / "bitsum.genes.tsv").exists()
    # genome_dist.tsv will be refreshed from EVERY sample's sequence: an old non-anchor sample whose FASTA is gone is a refusal
    # even when the new sample is no anchor, and nothing is touched
    tree = _tree_bytes(out)
    os.replace(tmp_path / "g1.fa", tmp_path / "g1.hidden")
    try:
        idx = pidx.Index(str(out), mode="w")
        with pytest.raises(ValueError, match="'g1'.*no longer there"):
            idx.add(pd.read_table(new_tsv).assign(anchor=False))
        idx.close()
    finally:
        os.replace(tmp_path / "g1.hidden", tmp_path / "g1.fa")
    assert _tree_bytes(out) == tree
    idx = pidx.Index(str(out), mode="w")
    idx.add(new_tsv)
    idx.close()
    fresh = _fresh(tmp_path, allp, k, genome_dist=True)
    assert (out / "anchor" / "g0" / "bitsum.genes.tsv").read_bytes() == (fresh / "anchor" / "g0" / "bitsum.genes.tsv").read_bytes()
    assert (out / "genome_dist.tsv").read_bytes() != before
    assert not (out / "kmer_shared.tsv").exists() and not (out / "anchor" / "g0" / "chrom_umaps.csv").exists()
    assert not (out / "anchor" / "g0" / "gene.bed.gz").exists()
    _same_index_payload(str(fresh), str(out))


def test_derived_files_that_were_there_are_refreshed(tmp_path):
    """kmer_shared.tsv / kmer_occupancy.tsv, genome_dist.tsv and an annotated anchor's gene and annotation tracks, all
    present before the add, are what a fresh index with the same switches holds"""
    from panagram_amd import index as pidx
    fx = H.load_case("n9_k21")
    k = int(fx["k"])
    gffs = {0: _gff_for(fx, 0, tmp_path)}
    (old_tsv, new_tsv), allp = _tables(tmp_path, fx, [8], gffs)
    out = tmp_path / "idx"
    switches = dict(genome_dist=True, kmer_stats=True, annotate=True)
    pidx.Index(old_tsv, prefix=str(out), k=k, **switches).run()
    for f in ("kmer_shared.tsv", "kmer_occupancy.tsv", "genome_dist.tsv", "anchor/g0/gene.bed.gz"):
        assert (out / f).exists(), f
    idx = pidx.Index(str(out), mode="w")
    idx.add(new_tsv)
    idx.close()
    assert "g8" in (out / "kmer_shared.tsv").read_text().splitlines()[0]
    _same_index_payload(str(_fresh(tmp_path, allp, k, **switches)), str(out))


def test_umap_files_that_were_there_are_refreshed(tmp_path):
    """chrom_umaps.csv and genome_umap.csv of an old anchor, written before the add, are afterwards what a fresh index of all
    samples with the same settings holds (their input is the pair counts of ALL samples' columns), and not what they were"""
    from panagram_amd import index as pidx
    k, lens, nbin = 21, [60_000, 61_300, 58_100], 2000
    gen = po.synth_genomes(4, lens, 0.02, 23)
    rows = []
    for g in range(4):
        fa = tmp_path / f"g{g}.fa"
        fa.write_bytes(po.fasta_text([f"chr{i + 1}" for i in range(len(lens))], [po.codes_to_ascii(c) for c in gen[g]]))
        rows.append((f"g{g}", str(fa), g == 0))
    for nm, part in (("old", rows[:3]), ("new", rows[3:]), ("all", rows)):
        pd.DataFrame(part, columns=["name", "fasta", "anchor"]).to_csv(tmp_path / f"{nm}.tsv", sep="\t", index=False)
    settings = dict(k=k, chrom_umap=pidx.UMAP(bin_size=nbin), genome_umap=pidx.UMAP(bin_size=nbin), umaps=True)
    out = tmp_path / "idx"
    pidx.Index(str(tmp_path / "old.tsv"), prefix=str(out), **settings).run()
    files = [out / "anchor" / "g0" / "chrom_umaps.csv", out / "anchor" / "g0" / "genome_umap.csv"]
    before = [f.read_bytes() for f in files]
    idx = pidx.Index(str(out), mode="w")
    assert idx.add(str(tmp_path / "new.tsv")) == ["rewrote anchor g0: 3 -> 4 samples"]
    idx.close()
    fresh = tmp_path / "fresh"
    pidx.Index(str(tmp_path / "all.tsv"), prefix=str(fresh), **settings).run()
    for f, was in zip(files, before):
        assert f.read_bytes() == (fresh / f.relative_to(out)).read_bytes(), f.name
        assert f.read_bytes() != was, f.name
        assert len(f.read_bytes().splitlines()) == len(was.splitlines())  # (the same bins)
    _same_index_payload(str(fresh), str(out))


def test_probe_without_direct_columns_and_out_of_memory(tmp_path, monkeypatch):
    """(a) a probe table that cannot emit columns itself goes through one-byte rows and extract_columns: the same tree;
    (b) an anchor whose new rows do not fit the free memory is refused before anything is written"""
    from panagram_amd import engine, index as pidx
    fx = H.load_case("n9_k21")
    k = int(fx["k"])
    (old_tsv, new_tsv), _ = _tables(tmp_path, fx, [8])
    out = tmp_path / "idx"
    pidx.Index(old_tsv, prefix=str(out), k=k).run()
    before = _tree_bytes(out)
    with monkeypatch.context() as m:
        m.setattr(engine.Context, "mem_info", lambda self: (64 << 20, 1 << 38))
        idx = pidx.Index(str(out), mode="w")
        try:
            with pytest.raises(MemoryError, match="free"):
                idx.add(new_tsv)
        finally:
            idx.close()
    assert _tree_bytes(out) == before
    direct = []
    real = engine.AnchorResult.columns_direct
    monkeypatch.setattr(engine.AnchorResult, "columns_direct", lambda self, width: direct.append(real(self, width)) and False)
    idx = pidx.Index(str(out), mode="w")
    idx.add(new_tsv)
    idx.close()
    assert direct and all(direct)  # (the tables did qualify: the other path was forced)
    _check_golden(out, fx)


def test_added_read_set_is_counted_with_ci2(tmp_path):
    """a FASTQ sample (never an anchor) added to an index enters the old anchor's rows with kmc -ci2 semantics, as it does
    in `index` (tests/test_gpu_index_e2e.py::test_fastq_sample_is_counted_with_ci2): the rows equal the oracle's; a
    FASTQ sample the table leaves an anchor is refused"""
    import gzip as gz
    from panagram_amd import index as pidx
    from tests.test_gpu_parity import _simulate_reads
    k = 21
    rng = np.random.default_rng(3)
    gen = po.synth_genomes(2, [9000, 4000], 0.02, 99)
    asm = [po.codes_to_ascii(c) for c in gen[0]]
    reads = _simulate_reads(rng, po.codes_to_ascii(gen[1][0]), 300, 120, 0.01)
    fa = tmp_path / "a.fa"
    fa.write_bytes(po.fasta_text(["c1", "c2"], asm))
    fq = tmp_path / "r.fq.gz"
    with gz.open(fq, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@r%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n")
    (tmp_path / "old.tsv").write_text(f"name\tfasta\tanchor\nasm\t{fa}\tTrue\n")
    out = tmp_path / "idx"
    pidx.Index(str(tmp_path / "old.tsv"), prefix=str(out), k=k).run()
    idx = pidx.Index(str(out), mode="w")
    with pytest.raises(ValueError, match="FASTQ sample cannot be an anchor"):
        idx.add(pd.DataFrame({"name": ["reads"], "fasta": [str(fq)]}))
    assert idx.add(pd.DataFrame({"name": ["reads"], "fasta": [str(fq)], "anchor": [False]})) == ["rewrote anchor asm: 1 -> 2 samples"]
    idx.close()
    dbs = po.build_bitvec_dbs([asm, reads], k, min_counts=[1, 2])
    want = b"".join(po.anchor_contig(dbs, s, k, 2)[0].tobytes() for s in asm)
    assert gzip.open(out / "anchor" / "asm" / "bitmap.1.gz").read() == want
    assert not (out / "anchor" / "reads").exists()
    assert list(pd.read_table(out / "samples.tsv")["name"]) == ["asm", "reads"]


def test_refusals_leave_the_tree_as_it_was(tmp_path, monkeypatch):
    from panagram_amd import index as pidx
    fx = H.load_case("n2_k21")
    k = int(fx["k"])
    (old_tsv, new_tsv), _ = _tables(tmp_path, fx, [1])
    out = tmp_path / "idx"
    pidx.Index(old_tsv, prefix=str(out), k=k).run()
    (out / ".add_staging").mkdir()  # (what a failed add left)
    (out / ".add_staging" / "junk").write_text("x")
    before = _tree_bytes(out)
    new = pd.read_table(new_tsv)

    def refused(table, match, mode="w", **kw):
        idx = pidx.Index(str(out), mode=mode, **kw)
        try:
            with pytest.raises(ValueError, match=match):
                idx.add(table)
        finally:
            idx.close()
        assert _tree_bytes(out) == before

    refused(new.assign(name="g0"), "already in the index")
    refused(new.assign(fasta=str(tmp_path / "nowhere.fa")), "no FASTA")
    refused(new.assign(name="bad name!"), "Invalid genome names")
    refused(new, "read-only", mode="r")
    refused(new, "one process", world=2)
    # an old anchor's inputs gone: its FASTA, its bitmap, its chrs.tsv (put back each time)
    a0 = f"g{int([g for g in fx['anchors'] if g < 1][0])}"
    for victim, match in ((tmp_path / f"{a0}.fa", "no longer there"), (out / "anchor" / a0 / "bitmap.1.gz", "bitmap.1.gz"),
                          (out / "anchor" / a0 / "chrs.tsv", "chrs.tsv")):
        hidden = victim.with_suffix(".hidden")
        os.replace(victim, hidden)
        try:
            idx = pidx.Index(str(out), mode="w")
            try:
                with pytest.raises(ValueError, match=match):
                    idx.add(new)
            finally:
                idx.close()
        finally:
            os.replace(hidden, victim)
        assert _tree_bytes(out) == before
    # a failure in the middle of the work: the tree is untouched, the staging directory gone
    from panagram_amd import add as padd
    monkeypatch.setattr(padd, "_move_tree", lambda *a: (_ for _ in ()).throw(RuntimeError("stop before the commit")))
    idx = pidx.Index(str(out), mode="w")
    try:
        with pytest.raises(RuntimeError, match="stop before the commit"):
            idx.add(new)
    finally:
        idx.close()
    after = _tree_bytes(out)
    assert {p: b for p, b in before.items() if not p.startswith(".add_staging")} == after


def test_add_cli(tmp_path, capsys):
    from panagram_amd import index as pidx
    from panagram_amd.__main__ import main
    fx = H.load_case("n2_k21")
    k = int(fx["k"])
    (old_tsv, new_tsv), allp = _tables(tmp_path, fx, [1])
    out = tmp_path / "idx"
    pidx.Index(old_tsv, prefix=str(out), k=k).run()
    capsys.readouterr()
    assert main(["add", str(out), new_tsv]) == 0
    printed = capsys.readouterr().out.splitlines()
    anchors = [int(g) for g in fx["anchors"]]
    assert printed == [f"rewrote anchor g{g}: 1 -> 2 samples" for g in anchors if g < 1] + [f"added anchor g{g}: 2 samples" for g in anchors if g >= 1]
    _check_golden(out, fx)
    with pytest.raises(SystemExit):
        main(["add", str(out), new_tsv])  # the names are in the index now
