"""CPU: genome_dist.tsv without a device — the restatement's MurmurHash3 against smhasher's known answers, mash's merge
against brute force, pg_minhash_distances (host only) against the restatement, the written file as the viewer reads it,
config.yaml with the new opt-in field, and the CLI."""
import os

import numpy as np
import pytest
import yaml

from tests import minhash_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_murmur3_known_answers(golden_dir):
    kat = np.load(os.path.join(golden_dir, "murmur3", "murmur3_kat.npz"))
    msg = kat["message"]
    assert len(kat["h1"]) == 82
    for seed, length, h1, h2 in zip(kat["seed"], kat["length"], kat["h1"], kat["h2"]):
        g1, g2 = ref.murmur3_x64_128(msg[None, :int(length)], int(seed))
        assert (int(g1[0]), int(g2[0])) == (int(h1), int(h2)), (int(seed), int(length))


def test_canonical_kmers_are_the_smaller_string():
    rng = np.random.default_rng(3)
    seq = bytes(rng.choice(np.frombuffer(b"ACGTacgtNR", np.uint8), 2000, p=[0.124] * 8 + [0.004] * 2))
    got = [bytes(r) for r in ref.canonical_kmers(seq, 21)]
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    want = []
    for i in range(len(seq) - 20):
        s = seq[i:i + 21].upper()
        if set(s) <= set(b"ACGT"):
            want.append(min(s, s.translate(comp)[::-1]))
    assert got == want and len(want) > 0


def _brute(a, b, s):
    union = sorted(set(int(x) for x in a) | set(int(x) for x in b))[:s]
    shared = set(int(x) for x in a) & set(int(x) for x in b)
    return sum(x in shared for x in union), len(union)


@pytest.mark.parametrize("seed", range(6))
def test_merge_is_s_smallest_of_the_union(seed):
    rng = np.random.default_rng(seed)
    s = int(rng.integers(5, 60))
    pool = np.unique(rng.integers(0, 2 ** 64, 400, dtype=np.uint64))
    cases = []
    for _ in range(20):
        a = np.unique(rng.choice(pool, int(rng.integers(0, 2 * s)), replace=False))[:s]
        b = np.unique(rng.choice(pool, int(rng.integers(0, 2 * s)), replace=False))[:s]
        cases.append((a, b))
    cases += [(pool[:s], pool[:s]), (pool[:s], pool[s:2 * s]), (pool[:3], pool[:s]), (pool[:0], pool[:s]), (pool[:0], pool[:0])]
    for a, b in cases:
        assert ref.compare(a, b, s) == _brute(a, b, s)


def _random_sketches(rng, n, s=ref.S):
    base = np.unique(rng.integers(0, 2 ** 64, 3 * s, dtype=np.uint64))
    out = []
    for i in range(n):
        keep = rng.random(base.size) < 0.2 + 0.7 * rng.random()
        extra = rng.integers(0, 2 ** 64, int(rng.integers(0, s)), dtype=np.uint64)
        out.append(np.unique(np.concatenate([base[keep], extra]))[:int(rng.integers(s // 3, s + 1))])
    return out


def test_host_distances_equal_the_restatement():
    from panagram_amd import engine
    rng = np.random.default_rng(11)
    sk = _random_sketches(rng, 9)
    sk += [sk[2].copy(), np.zeros(0, np.uint64), np.sort(rng.integers(0, 2 ** 64, 40, dtype=np.uint64))]
    bases = [int(x) for x in rng.integers(10 ** 4, 4 * 10 ** 9, len(sk))]
    dist, pval, common, denom = engine.minhash_distances(sk, bases)
    want = ref.pairs(sk, bases)
    assert len(want) == len(dist) == len(sk) * (len(sk) - 1) // 2
    for t, (i, j, d, p, c, n) in enumerate(want):
        assert (int(common[t]), int(denom[t])) == (c, n), (i, j)
        assert dist[t] == d and pval[t] == p, (i, j, dist[t], d, pval[t], p)  # the same arithmetic: equal bits


def test_host_distances_small_s_and_no_pairs():
    from panagram_amd import engine
    a = np.array([1, 5, 9, 12], np.uint64)
    b = np.array([1, 6, 9, 13], np.uint64)
    dist, pval, common, denom = engine.minhash_distances([a, b], None, s=3)
    assert (int(common[0]), int(denom[0])) == ref.compare(a, b, 3) == (1, 3)
    assert dist[0] == ref.distance(1, 3) and pval[0] == 1.0
    assert all(len(x) == 0 for x in engine.minhash_distances([a], [100]))


def _index(tmp_path, names, out="out", **kw):
    from panagram_amd.index import Index
    tsv = tmp_path / "samples.tsv"
    tsv.write_text("name\tfasta\n" + "".join(f"{n}\t{tmp_path / (n + '.fa')}\n" for n in names))
    return Index(str(tsv), prefix=str(tmp_path / out), **kw)


def test_written_file_reads_like_the_viewer(tmp_path):
    """the loop of the reference's figs.make_all_genome_dend (panagram/figs.py:53-59) on the file"""
    names = ["g0", "g1", "g2", "g3", "g4"]
    idx = _index(tmp_path, names)
    rng = np.random.default_rng(5)
    sk = _random_sketches(rng, len(names))
    bases = [int(x) for x in rng.integers(10 ** 6, 10 ** 9, len(names))]
    idx._minhash = {n: (sk[i], bases[i]) for i, n in enumerate(names)}
    path = idx.write_genome_dist()
    assert path == os.path.join(str(tmp_path / "out"), "genome_dist.tsv")
    text = open(path).read()
    assert text == ref.genome_dist_text(names, sk, bases)
    ids = {n: g.id for n, g in idx.genomes.items()}
    dist_mat = np.zeros((idx.ngenomes, idx.ngenomes), np.float64)
    with open(idx.genome_dist_fname) as f:
        for line in f:
            f, t, d, p, x = line.rstrip().split("\t")
            i = ids[f]
            j = ids[t]
            dist_mat[i][j] = d
            dist_mat[j][i] = d
    assert np.array_equal(dist_mat, dist_mat.T) and not np.diag(dist_mat).any()
    assert (dist_mat + np.eye(len(names)) > 0).all()
    assert len(text.splitlines()) == len(names) * (len(names) - 1) // 2
    idx.close()


def test_config_yaml_unchanged_by_the_flag(tmp_path):
    off = _index(tmp_path, ["x", "y"], out="a")
    on = _index(tmp_path, ["x", "y"], out="b", genome_dist=True)
    assert on.genome_dist and not off.genome_dist
    a, b = open(off.config_fname).read(), open(on.config_fname).read()
    assert a == b and "genome_dist" not in yaml.safe_load(a)
    off.close()
    on.close()


def test_cli_parses_genome_dist_and_dist(monkeypatch, tmp_path):
    from panagram_amd import __main__ as cli
    from panagram_amd import index as index_mod
    seen = []

    class FakeIndex:
        def __init__(self, input, **kw):
            seen.append((input, kw))
            self.kw = kw

        def run(self):
            seen.append("run")

        def write_genome_dist(self):
            seen.append("write_genome_dist")
            return "genome_dist.tsv"

        def close(self):
            seen.append("close")

    monkeypatch.setattr(index_mod, "Index", FakeIndex)
    assert cli.main(["index", "s.tsv", "-k", "31", "--genome_dist"]) == 0
    assert seen[0][0] == "s.tsv" and seen[0][1]["genome_dist"] is True and seen[0][1]["k"] == 31 and seen[1] == "run"
    seen.clear()
    assert cli.main(["index", "s.tsv"]) == 0
    assert seen[0][1]["genome_dist"] is False
    seen.clear()
    assert cli.main(["dist", str(tmp_path), "--device", "0"]) == 0
    assert seen[0] == (str(tmp_path), {"mode": "r", "device": 0}) and seen[1:] == ["write_genome_dist", "close"]
