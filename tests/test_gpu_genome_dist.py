"""GPU: MinHash sketches taken on the device (pg_minhash_*, engine.MinHashSketch) equal the restatement
(tests/minhash_ref.py), whichever path the candidates took; genome_dist.tsv written by Index.run(genome_dist=True), by
several ranks and by the `dist` command is the file the restatement predicts."""
import os

import numpy as np
import pytest

from tests import helpers as H
from tests import minhash_ref as ref

pytestmark = pytest.mark.gpu


def _gpu_sketch(ctx, records, **kw):
    from panagram_amd import engine
    ss = engine.SeqSet.from_host(ctx, records)
    hll = engine.KmerSketch(ctx, 21)
    hll.add(ss)
    mh = engine.MinHashSketch(ctx, **kw)
    mh.add(ss, hll.estimate())
    out, bases = mh.result()
    passes = mh.passes()
    for o in (mh, hll, ss):
        o.close()
    return out, bases, passes


def _random(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(alphabet, np.uint8), n))


def _edge_records(rng):
    recs = []
    a = bytearray(_random(rng, 30000))
    a[1000:1040] = b"N" * 40                          # an N run
    for p in rng.integers(2000, 29000, 40):           # IUPAC codes and stray bytes
        a[int(p)] = b"RYKMSWBDHVN-"[int(p) % 12]
    recs.append(bytes(a))
    b = bytearray(_random(rng, 12000))
    b[500:9000] = bytes(b[500:9000]).lower()          # lower case
    recs.append(bytes(b))
    recs += [_random(rng, int(x)) for x in (1, 5, 20)]  # shorter than k
    recs.append(_random(rng, 21))                      # exactly one k-mer
    half = _random(rng, 400)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    recs.append(half + half.translate(comp)[::-1])   # a reverse-complement palindrome
    recs.append(b"ACGT" * 200 + b"AT" * 100)          # palindromic repeats
    recs += [_random(rng, int(x)) for x in rng.integers(21, 300, 300)]  # many records
    return recs


def test_sketch_equals_restatement_edge_cases(ctx):
    rng = np.random.default_rng(21)
    recs = _edge_records(rng)
    got, bases, passes = _gpu_sketch(ctx, recs)
    want = ref.sketch(recs)
    assert len(want) == ref.S
    assert np.array_equal(got, want)
    assert bases == ref.acgt_bases(recs)
    assert passes == 1


def test_sketch_of_few_kmers_keeps_them_all(ctx):
    rng = np.random.default_rng(4)
    recs = [_random(rng, 3000), b"acgtnacgt" * 30, _random(rng, 19)]
    got, bases, _ = _gpu_sketch(ctx, recs)
    want = ref.sketch(recs)
    assert 0 < len(want) < ref.S and np.array_equal(got, want)
    assert bases == ref.acgt_bases(recs)
    empty, nb, _ = _gpu_sketch(ctx, [b"NNNNNNNNNNNNNNNNNNNNNNNNN", b"ACGT"])
    assert len(empty) == 0 and nb == 4


@pytest.mark.parametrize("kw", [dict(tau=1 << 44), dict(capacity=64), dict(tau=1 << 40, capacity=16)])
def test_forced_fallbacks_give_the_same_sketch(ctx, kw):
    """a threshold too low (reruns at 4 tau) and a buffer too small (reruns with a 4x buffer) change nothing"""
    rng = np.random.default_rng(8)
    recs = _edge_records(rng)[:3] + [_random(rng, 40000)]
    auto, _, p_auto = _gpu_sketch(ctx, recs)
    forced, _, p_forced = _gpu_sketch(ctx, recs, **kw)
    assert np.array_equal(forced, auto) and np.array_equal(auto, ref.sketch(recs))
    assert p_auto == 1 and p_forced > 1


def test_fastq_sample(ctx, tmp_path):
    from panagram_amd import engine
    from panagram_amd.index import read_fastq_joined
    rng = np.random.default_rng(6)
    genome = _random(rng, 20000)
    reads = []
    for p in rng.integers(0, 20000 - 150, 400):
        r = bytearray(genome[int(p):int(p) + 150])
        if p % 3 == 0:
            r[70] = ord("N")
        reads.append(bytes(r))
    fq = tmp_path / "r.fq"
    fq.write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads)))
    ss = engine.SeqSet.from_host(ctx, [read_fastq_joined(str(fq))])
    mh = engine.MinHashSketch(ctx)
    mh.add(ss)
    got, bases = mh.result()
    mh.close()
    ss.close()
    assert np.array_equal(got, ref.sketch(reads))
    assert bases == ref.acgt_bases(reads)


def test_several_seqsets_make_one_sketch(ctx):
    from panagram_amd import engine
    rng = np.random.default_rng(12)
    parts = [[_random(rng, 9000), _random(rng, 300)], [_random(rng, 15000)]]
    mh = engine.MinHashSketch(ctx)
    for recs in parts:
        ss = engine.SeqSet.from_host(ctx, recs)
        mh.add(ss)
        ss.close()
    got, bases = mh.result()
    mh.close()
    assert np.array_equal(got, ref.sketch(parts[0] + parts[1])) and bases == ref.acgt_bases(parts[0] + parts[1])


def _write_case(tmp_path, fx):
    rows = ["name\tfasta"]
    for g in range(int(fx["ngenomes"])):
        fa = tmp_path / f"g{g}.fa"
        fa.write_bytes(fx[f"fasta_{g}"].tobytes())
        rows.append(f"g{g}\t{fa}")
    s = tmp_path / "samples.tsv"
    s.write_text("\n".join(rows) + "\n")
    return s


def _predicted(fx, tmp_path):
    """the file the restatement predicts for the samples of a fixture (records as the host's FASTA reader splits them)"""
    from panagram_amd.index import read_fasta
    names, sketches, bases = [], [], []
    for g in range(int(fx["ngenomes"])):
        recs = [seq for _, seq in read_fasta(str(tmp_path / f"g{g}.fa"))]
        names.append(f"g{g}")
        sketches.append(ref.sketch(recs))
        bases.append(ref.acgt_bases(recs))
    return ref.genome_dist_text(names, sketches, bases)


def test_index_run_writes_predicted_genome_dist_k31(tmp_path):
    """an index with k = 31 still gets 21-mer distances; the file is the restatement's, byte for byte"""
    from panagram_amd import index as pidx
    fx = H.load_case("n40_k31")
    s = _write_case(tmp_path, fx)
    out = tmp_path / "idx"
    idx = pidx.Index(str(s), prefix=str(out), k=int(fx["k"]), anchor_genomes=[f"g{g}" for g in fx["anchors"]], genome_dist=True)
    idx.run()
    text = (out / "genome_dist.tsv").read_text()
    assert text == _predicted(fx, tmp_path)
    n = int(fx["ngenomes"])
    mat = np.zeros((n, n))
    for line in text.splitlines():
        f, t, d, p, x = line.rstrip().split("\t")
        mat[int(f[1:]), int(t[1:])] = mat[int(t[1:]), int(f[1:])] = float(d)
    assert np.array_equal(mat, mat.T) and not np.diag(mat).any() and len(text.splitlines()) == n * (n - 1) // 2


@pytest.mark.parametrize("partition", ["pieces", "genomes"])
def test_ranks_and_dist_command_write_the_same_file(partition, tmp_path, monkeypatch):
    """world 2 (the ranks one after the other): only rank 0 writes, the same bytes as one rank; and `dist` on an index
    built without the flag rewrites them"""
    from panagram_amd import __main__ as cli
    from panagram_amd import index as pidx
    monkeypatch.setenv("PG_PARTITION", partition)
    fx = H.load_case("n9_k21")
    k = int(fx["k"])
    anchors = [f"g{g}" for g in fx["anchors"]]
    s = _write_case(tmp_path, fx)
    one = tmp_path / "one"
    pidx.Index(str(s), prefix=str(one), k=k, anchor_genomes=anchors, genome_dist=True).run()
    want = (one / "genome_dist.tsv").read_bytes()
    assert want.decode() == _predicted(fx, tmp_path)
    many = tmp_path / "many"
    pidx.Index(str(s), prefix=str(many), k=k, anchor_genomes=anchors, rank=0, world=2, genome_dist=True).run()
    got = (many / "genome_dist.tsv").read_bytes()
    os.remove(many / "genome_dist.tsv")
    pidx.Index(str(s), prefix=str(many), k=k, anchor_genomes=anchors, rank=1, world=2, genome_dist=True).run()
    assert not (many / "genome_dist.tsv").exists() and got == want
    plain = tmp_path / "plain"
    pidx.Index(str(s), prefix=str(plain), k=k, anchor_genomes=anchors).run()
    assert not (plain / "genome_dist.tsv").exists()
    assert cli.main(["dist", str(plain)]) == 0
    assert (plain / "genome_dist.tsv").read_bytes() == want


def test_distance_tracks_divergence(ctx):
    """8 genomes of 300 kb, each pair 1 % apart per base (each 0.5 % from a common ancestor): D within 20 % of 0.01"""
    from panagram_amd import engine
    rng = np.random.default_rng(17)
    anc = np.frombuffer(_random(rng, 300000), np.uint8)
    d = 0.01
    sketches = []
    mh = engine.MinHashSketch(ctx)
    for g in range(8):
        x = anc.copy()
        hit = np.flatnonzero(rng.random(x.size) < d / 2)
        x[hit] = np.frombuffer(b"ACGT", np.uint8)[(np.searchsorted(np.frombuffer(b"ACGT", np.uint8), x[hit]) + rng.integers(1, 4, hit.size)) % 4]
        ss = engine.SeqSet.from_host(ctx, [x.tobytes()])
        mh.reset()
        mh.add(ss)
        sketches.append(mh.result()[0])
        ss.close()
    mh.close()
    dist = engine.minhash_distances(sketches, [300000] * 8)[0]
    assert dist.size == 28 and np.all(np.abs(dist - d) < 0.2 * d), dist
