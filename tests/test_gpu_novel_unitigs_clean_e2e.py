"""GPU: `novel --unitigs --clean` and Index.novel(..., clean=...) end to end on the index of tests/test_gpu_novel_e2e.py and reads of
the first contig of its planted sample: error-free reads tiled at 20-fold on random strands, and four substitutions inside the
planted insertion, each carried by exactly two reads — two in the middle of their reads (bubbles of k k-mers at depth 2), two
within k of their reads' ends (tips).  Without --clean the insertion comes back in pieces, with it as exactly the one unitig of
tests/unitigs_ref.e2e_insertion; the five statistic lines are the model's."""
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
from tests import unitigs_clean_ref as CR
from tests import unitigs_ref as UR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = pr.E2E["k"]
READ, STRIDE = 100, 5                   # every interior base lies in 20 reads
BUBBLES, TIPS = (100, 200), (300, 400)  # offsets into the insertion
MC = 2


def e2e_clean_reads():
    """the reads: the sample's first contig tiled, then two reads per planted error"""
    c0 = NR.e2e_sample()[0]
    rng = np.random.default_rng(pr.E2E["seed"] + 21)
    reads = [c0[s:s + READ] for s in range(0, len(c0) - READ + 1, STRIDE)]

    def bad(at, offsets):
        x = NR.E2E_INS_AT + at
        other = bytes([b"ACGT"[(b"ACGT".index(c0[x]) + 1 + int(rng.integers(0, 3))) % 4]])
        for o in offsets:  # (the error at base o of its read)
            r = c0[x - o:x - o + READ]
            reads.append(r[:o] + other + r[o + 1:])
    for at in BUBBLES:
        bad(at, (40, 60))
    for at in TIPS:
        bad(at, (READ - 5, READ - 6))
    return [r if rng.random() < 0.5 else SR.revcomp(r) for r in reads]


def model():
    """(raw nodes, cleaned nodes, the model's statistics) at min_count 2"""
    _, _, nk, d = NR.novel_counts(SR.e2e_table()[0], [pr.joined_reads(e2e_clean_reads())], K)
    raw = UR.nodes_of(nk, d, MC)
    left, st = CR.clean(raw, K)
    return raw, left, st


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    from panagram_amd import index as pidx
    tmp = tmp_path_factory.mktemp("clean")
    genomes, _ = pr.e2e_genomes()
    lines = ["name\tfasta\tgff"]
    for name, contigs in zip(pr.E2E_NAMES, genomes):
        fa = tmp / f"{name}.fa"
        fa.write_bytes(po.fasta_text(pr.E2E_CHROMS, contigs))
        lines.append(f"{name}\t{fa}\t")
    (tmp / "samples.tsv").write_text("\n".join(lines) + "\n")
    out = str(tmp / "idx")
    pidx.Index(str(tmp / "samples.tsv"), prefix=out, k=K, anchor_genomes=["A"], lowres_step=100).run()
    fq = str(tmp / "reads.fq")
    with open(fq, "wb") as f:
        f.write(pr.fastq_text(e2e_clean_reads()))
    return out, fq


def test_the_insertion_comes_back_whole_with_clean(built, tmp_path):
    from panagram_amd import index as pidx
    out, fq = built
    raw, left, want = model()
    ins = UR.e2e_insertion()
    rawU, cleanU = UR.unitigs(raw, K), UR.unitigs(left, K)
    assert ins not in {s for s, _, _, _ in rawU} and ins in {s for s, _, _, _ in cleanU}  # (the premise, under the model)
    assert want["clipped_tips"] == len(TIPS) and want["popped_bubbles"] == len(BUBBLES) and want["popped_kmers"] == K * len(BUBBLES)
    idx = pidx.Index(out, mode="r")
    try:
        got = idx.novel(fq, unitigs=True)
        assert len(got) == 5 and got[0]["min_count"] == MC
        frame = got[4]
        assert ins not in frame["sequence"].tolist()
        pieces = [s for s in frame["sequence"] if s in ins or UR.revcomp(s) in ins]
        assert len(pieces) > 1  # the insertion in more than one unitig
        assert set(zip(frame["sequence"], frame["kmers"])) == {(s, n) for s, n, _, _ in rawU}
        got = idx.novel(fq, unitigs=True, clean={})
        assert len(got) == 6 and got[5] == want
        frame = got[4]
        hit = frame[frame["sequence"] == ins]
        assert len(hit) == 1 and int(hit["kmers"].iloc[0]) == NR.E2E_INSERTION + K - 1
        assert set(zip(frame["sequence"], frame["kmers"])) == {(s, n) for s, n, _, _ in cleanU}
        assert idx.novel(fq, unitigs=True, clean={"rounds": 0})[5] == dict(zip(CR.STAT_NAMES, [0] * 5))
        for bad in ({"ratio": 1.0}, {"tip_kmers": 0}, {"nonsense": 1}):
            with pytest.raises(ValueError, match="clean"):
                idx.novel(fq, unitigs=True, clean=bad)
        with pytest.raises(ValueError, match="clean needs unitigs"):
            idx.novel(fq, clean={})
    finally:
        idx.close()
    # the command in a child process: the unitig file, and the five lines behind what it prints without --clean
    fa, fc = tmp_path / "u.fa", tmp_path / "c.fa"
    base = ["timeout", "-k", "10", "240", sys.executable, "-m", "panagram_amd", "novel", out, fq]
    plain = subprocess.run(base + ["--unitigs", str(fa)], cwd=ROOT, capture_output=True, text=True)
    assert plain.returncode == 0, plain.stderr[-2000:]
    r = subprocess.run(base + ["--unitigs", str(fc), "--clean"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[-5:] == nov.clean_stat_lines(want) and len(lines) == len(plain.stdout.splitlines()) + 5
    assert lines[:len(lines) - 10] == plain.stdout.splitlines()[:-5]  # (the novel statistics; the unitig statistics differ)
    seqs = [b.replace("\n", "") for _, b in (x.split("\n", 1) for x in fc.read_text().split(">")[1:])]
    assert seqs.count(ins) == 1 and set(seqs) == {s for s, _, _, _ in cleanU}
    assert ins not in fa.read_text().replace("\n", "")
