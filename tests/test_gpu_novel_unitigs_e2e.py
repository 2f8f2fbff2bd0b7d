"""GPU: Index.novel(..., unitigs=True) and `novel --unitigs` on the index and the samples of tests/test_gpu_novel_e2e.py: A, B and C,
and genome B with a planted insertion, a substitution, a deletion and a wholly novel contig, as a FASTA and as reads of it.  No novel
k-mer of that assembly repeats (tests/test_unitigs_cpu.py proves it on the model), so its unitigs are its novel regions' slices; of
the reads the planted insertion comes back as one unitig; the command writes FASTA that parses back to the frame, its stdout begins
with what it prints without the flag; and without ``unitigs`` Index.novel returns its four values as before."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle as po
from panagram_amd import novel as nov
from tests import novel_ref as NR
from tests import place_ref as pr
from tests import screen_ref as SR
from tests import unitigs_ref as UR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = pr.E2E["k"]


def same(got, want, tag):
    """(stats, spectrum, kmers, regions) as tests/test_gpu_novel_e2e.py compares them"""
    assert list(got[0]) == nov.STAT_NAMES
    for key in nov.STAT_NAMES:
        assert got[0][key] == want[0][key], (tag, key, got[0][key], want[0][key])
    for g, w, what in zip(got[1:], want[1:], ("spectrum", "kmers", "regions")):
        assert (g is None) == (w is None), (tag, what)
        if w is not None:
            assert g.to_csv(sep="\t") == w.to_csv(sep="\t"), (tag, what)


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """the index, the FASTA sample and the two read files of tests/test_gpu_novel_e2e.py"""
    from panagram_amd import index as pidx
    tmp = tmp_path_factory.mktemp("unitigs")
    genomes, _ = pr.e2e_genomes()
    lines = ["name\tfasta\tgff"]
    for name, contigs in zip(pr.E2E_NAMES, genomes):
        fa = tmp / f"{name}.fa"
        fa.write_bytes(po.fasta_text(pr.E2E_CHROMS, contigs))
        lines.append(f"{name}\t{fa}\t")
    (tmp / "samples.tsv").write_text("\n".join(lines) + "\n")
    out = str(tmp / "idx")
    pidx.Index(str(tmp / "samples.tsv"), prefix=out, k=K, anchor_genomes=["A"], lowres_step=100).run()
    sample = tmp / "sample.fa"
    sample.write_bytes(po.fasta_text(NR.E2E_SAMPLE_NAMES, NR.e2e_sample()))
    reads = NR.e2e_reads()[0]
    h = len(reads) // 2
    r1, r2 = str(tmp / "reads_1.fq"), str(tmp / "reads_2.fq.gz")
    with open(r1, "wb") as f:
        f.write(pr.fastq_text(reads[:h]))
    with gzip.open(r2, "wb") as f:
        f.write(pr.fastq_text(reads[h:]))
    return out, str(sample), [r1, r2]


def model_frame(contigs, min_count, min_unitig_bases=0):
    """the frame of the model's unitigs"""
    _, _, nk, d = NR.novel_counts(SR.e2e_table()[0], [contigs], K)
    U = sorted(UR.unitigs(UR.nodes_of(nk, d, min_count), K))
    text = "".join(seq for seq, _, _, _ in U)
    offsets = [0]
    for seq, _, _, _ in U[:-1]:
        offsets.append(offsets[-1] + len(seq))
    return nov.unitigs_frame(offsets[:len(U)], [n for _, n, _, _ in U], [ds for _, _, ds, _ in U], [c for _, _, _, c in U],
                             np.frombuffer(text.encode(), np.uint8), K, min_unitig_bases)


def test_unitigs_of_the_assembly_and_of_its_reads(built):
    from panagram_amd import index as pidx
    out, sample, reads = built
    idx = pidx.Index(out, mode="r")
    try:
        got = idx.novel(sample, kmers=True, regions=True, unitigs=True)
        assert len(got) == 5
        same(got[:4], NR.e2e_model("fasta", 1, file=sample), "the assembly, with unitigs")
        regions, frame = got[3], got[4]
        contigs = dict(zip(NR.E2E_SAMPLE_NAMES, NR.e2e_sample()))
        slices = {nov.canonical_unitig(contigs[r.contig][r.start:r.end].decode()) for r in regions.itertuples(index=False)}
        assert set(frame["sequence"]) == slices and len(frame) == len(regions) == 4 and not frame["circular"].any()
        assert frame.to_csv(sep="\t") == model_frame(NR.e2e_sample(), 1).to_csv(sep="\t")
        assert frame["unitig"].tolist() == ["u1", "u2", "u3", "u4"] and frame["bases"].tolist() == sorted(frame["bases"], reverse=True)
        assert frame["bases"].tolist()[0] == NR.E2E_NOVEL_CONTIG and (frame["depth"] == 1.0).all()
        long_only = idx.novel(sample, unitigs=True, min_unitig_bases=1000)[4]
        assert long_only["sequence"].tolist() == frame["sequence"].tolist()[:1] and long_only["unitig"].tolist() == ["u1"]
        # the reads at their default threshold: the insertion in one piece, the frame the model's
        got = idx.novel(reads, unitigs=True)
        assert len(got) == 5 and got[0]["min_count"] == 2 and got[2] is None and got[3] is None
        same(got[:4], (*NR.e2e_model("reads", 2)[:2], None, None), "the reads, with unitigs")
        ins = UR.e2e_insertion()
        hit = got[4][got[4]["sequence"] == ins]
        assert len(hit) == 1 and int(hit["kmers"].iloc[0]) == NR.E2E_INSERTION + K - 1 and float(hit["depth"].iloc[0]) >= 2.0
        assert got[4].to_csv(sep="\t") == model_frame(pr.joined_reads(NR.e2e_reads()[0]), 2).to_csv(sep="\t")
        # without the flag: four values, the same as before
        plain = idx.novel(sample, kmers=True, regions=True)
        assert len(plain) == 4
        same(plain, NR.e2e_model("fasta", 1, file=sample), "the assembly, without unitigs")
        with pytest.raises(ValueError, match="min_unitig_bases"):
            idx.novel(sample, unitigs=True, min_unitig_bases=-1)
    finally:
        idx.close()


def test_novel_unitigs_subcommand_in_a_child_process(built, tmp_path):
    out, sample, reads = built
    fa = tmp_path / "u.fa"
    base = ["timeout", "-k", "10", "240", sys.executable, "-m", "panagram_amd", "novel", out, *reads, "--min-count", "2"]
    plain = subprocess.run(base, cwd=ROOT, capture_output=True, text=True)
    assert plain.returncode == 0, plain.stderr[-2000:]
    r = subprocess.run(base + ["--unitigs", str(fa), "--min-unitig-bases", "50"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    frame = model_frame(pr.joined_reads(NR.e2e_reads()[0]), 2, 50)
    # (the filter bites: the substitution's unitig has 2 k - 1 bases, the deletion's junction 2 k - 2)
    assert 2 <= len(frame) < len(model_frame(pr.joined_reads(NR.e2e_reads()[0]), 2)) and fa.read_text() == nov.unitig_fasta(frame)
    recs = [x.split("\n", 1) for x in fa.read_text().split(">")[1:]]
    assert [h.split()[0] for h, _ in recs] == frame["unitig"].tolist() and [b.replace("\n", "") for _, b in recs] == frame["sequence"].tolist()
    assert [h for h, _ in recs] == [nov.unitig_header(row)[1:] for row in frame.itertuples(index=False)]
    assert UR.e2e_insertion() in frame["sequence"].tolist()
    # stdout: exactly the lines of the command without the flag, the unitig statistics behind them
    assert plain.stdout == "".join(line + "\n" for line in nov.stat_lines(NR.e2e_model("reads", 2)[0]))
    assert r.stdout == plain.stdout + "".join(line + "\n" for line in nov.unitig_stat_lines(nov.unitig_stats(frame)))
    # --min-unitig-bases alone: refused before any work
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "panagram_amd", "novel", out, reads[0], "--min-unitig-bases", "50"], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 2 and "needs --unitigs" in r.stderr
