"""CPU: the pan-genome k-mer statistics' host side — the numpy reference against Python sets, pangenome.exact_distances and
pangenome.frames on hand-made arrays, the exact genome_dist.tsv lines, and the command line's argument errors."""
import itertools
import math

import numpy as np
import pandas as pd
import pytest

from oracle import pyoracle as po
from panagram_amd import pangenome
from tests import kmerstats_ref as KR
from tests import minhash_ref as MR

K = 21
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _kmer_set(seqs, k):
    out = set()
    for s in seqs:
        for i in range(len(s) - k + 1):
            w = s[i:i + k]
            if set(w) <= set(b"ACGT"):
                out.add(min(w, w.translate(_COMP)[::-1]))
    return out


def test_reference_equals_python_sets_on_three_small_genomes():
    genomes = [[po.codes_to_ascii(c) for c in g] for g in po.synth_genomes(3, [300], 0.05, 11)]
    genomes[2][0] = genomes[2][0][:150] + b"N" + genomes[2][0][151:]  # (k-mers over an N are no k-mers)
    sets = [_kmer_set(g, K) for g in genomes]
    keys, M = KR.from_groups(po.build_bitvec_dbs(genomes, K), 3)
    ref = KR.stats(keys, M)
    union = set().union(*sets)
    assert ref["nkeys"] == len(union) and len(union) > 300
    for a in range(3):
        for b in range(3):
            assert ref["pairs"][a, b] == len(sets[a] & sets[b])
    held = [sum(x in s for s in sets) for x in union]
    assert ref["occupancy"].tolist() == [held.count(n) for n in range(4)] and ref["occupancy"][0] == 0
    assert ref["private"].tolist() == [len(sets[g] - set().union(*(sets[o] for o in range(3) if o != g))) for g in range(3)]
    assert 0 < ref["occupancy"][3] < len(union) and all(ref["private"] > 0)  # the input stays non-trivial
    # and the group words round-trip
    words = KR.group_words(M)
    assert len(words) == 1 and np.array_equal(KR.from_groups([(keys, words[0])], 3)[1], M)


def test_random_keys_are_distinct_canonical_kmers():
    keys = KR.random_keys(np.random.default_rng(3), 500, K)
    assert len(np.unique(keys)) == 500
    for key in keys[:50]:
        s = bytes(b"ACGT"[(int(key) >> (2 * (K - 1 - i))) & 3] for i in range(K))
        assert s <= s.translate(_COMP)[::-1]
        kk, valid = po.canonical_kmers(s, K)
        assert valid.all() and int(kk[0]) == int(key)


def test_exact_distances_limits_symmetry_and_the_mash_formula():
    #            a    b    c    d(empty)  e (= a)
    c = np.array([[100, 40, 0, 0, 100],
                  [40, 80, 0, 0, 40],
                  [0, 0, 50, 0, 0],
                  [0, 0, 0, 0, 0],
                  [100, 40, 0, 0, 100]], np.int64)
    j, d = pangenome.exact_distances(c, K)
    order = list(itertools.combinations(range(5), 2))
    assert len(j) == len(d) == 10
    at = {p: i for i, p in enumerate(order)}
    assert j[at[(0, 4)]] == 1.0 and d[at[(0, 4)]] == 0.0  # identical sets
    assert j[at[(0, 2)]] == 0.0 and d[at[(0, 2)]] == 1.0  # disjoint sets
    for other in (0, 1, 2):  # a genome without k-mers shares nothing
        assert j[at[(other, 3)]] == 0.0 and d[at[(other, 3)]] == 1.0
    assert j[at[(3, 4)]] == 0.0 and d[at[(3, 4)]] == 1.0
    assert j[at[(0, 1)]] == 40 / 140
    assert d[at[(0, 1)]] == pytest.approx(-math.log(2 * (40 / 140) / (1 + 40 / 140)) / K, rel=1e-15)
    # symmetry: the transposed matrix, and the genomes in another order
    j2, d2 = pangenome.exact_distances(c.T.copy(), K)
    assert np.array_equal(j, j2) and np.array_equal(d, d2)
    perm = [4, 2, 0, 3, 1]
    jp, dp = pangenome.exact_distances(c[np.ix_(perm, perm)], K)
    for t, (x, y) in enumerate(order):
        a, b = sorted((perm[x], perm[y]))
        assert jp[t] == j[at[(a, b)]] and dp[t] == d[at[(a, b)]]
    # the distance formula of the MinHash reference, fed the same j
    for k in (15, 21, 31):
        for common, denom in [(0, 10), (10, 10), (1, 10000), (9999, 10000), (40, 140), (1, 10 ** 12), (123456, 7654321)]:
            m = np.array([[denom, common], [common, common]], np.int64)  # shared = common, union = denom
            jj, dd = pangenome.exact_distances(m, k)
            assert jj[0] == common / denom
            assert dd[0] == pytest.approx(MR.distance(common, denom, k), rel=1e-14, abs=0)
    assert all(len(x) == 0 for x in pangenome.exact_distances(np.array([[7]]), K))


def test_frames_columns_add_up_to_the_occupancy():
    rng = np.random.default_rng(8)
    for n in (2, 5, 33):
        M = (rng.random((4000, n)) < rng.random(n)).astype(np.uint8)
        M[:40] = 1
        M = M[M.any(axis=1)]
        ref = KR.stats(np.arange(len(M), dtype=np.uint64), M)
        names = [f"s{i}" for i in range(n)]
        shared, genomes = pangenome.frames(ref, names)
        occ = ref["occupancy"]
        assert list(shared.index) == list(shared.columns) == names and shared.index.name == "name"
        assert np.array_equal(shared.to_numpy(), ref["pairs"]) and np.array_equal(shared.to_numpy(), shared.to_numpy().T)
        assert list(genomes.columns) == ["kmers", "private", "core", "shell"] and list(genomes.index) == names
        assert np.array_equal(genomes["kmers"].to_numpy(), np.diag(ref["pairs"]))
        assert (genomes["core"] == occ[n]).all() and occ[n] >= 40
        assert np.array_equal(genomes["private"] + genomes["shell"] + genomes["core"], genomes["kmers"])
        assert (genomes["shell"] >= 0).all()
        assert genomes["private"].sum() == occ[1]
        assert genomes["core"].sum() == n * occ[n]
        assert genomes["shell"].sum() == sum(i * occ[i] for i in range(2, n))
        assert genomes["kmers"].sum() == sum(i * occ[i] for i in range(n + 1))
        of = pangenome.occupancy_frame(ref)
        assert list(of.columns) == ["n", "kmers"] and of["n"].tolist() == list(range(n + 1)) and of["kmers"].tolist() == occ.tolist()
    with pytest.raises(ValueError):
        pangenome.frames(ref, names[:-1])


def test_exact_genome_dist_lines_layout_and_pair_order(tmp_path):
    names = ["b", "a", "c"]  # sample order, not sorted
    c = np.array([[1000, 250, 0], [250, 500, 500], [0, 500, 2000]], np.int64)
    lines = pangenome.genome_dist_lines(names, c, K)
    d_ba = -math.log(2 * 0.2 / 1.2) / K
    d_ac = -math.log(2 * 0.25 / 1.25) / K
    assert lines == [f"b\ta\t{d_ba:.6g}\t0\t250/1250\n", "b\tc\t1\t0\t0/3000\n", f"a\tc\t{d_ac:.6g}\t0\t500/2000\n"]
    # read like today's file (figs.py:50-59 reads the names and the distance)
    f = tmp_path / "genome_dist.tsv"
    f.write_text("".join(lines))
    got = pd.read_table(f, names=["a", "b", "dist", "p", "frac"])
    assert got[["a", "b"]].values.tolist() == [["b", "a"], ["b", "c"], ["a", "c"]]
    assert got["dist"].tolist() == [float(f"{d_ba:.6g}"), 1.0, float(f"{d_ac:.6g}")] and got["p"].tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        pangenome.genome_dist_lines(names[:2], c, K)


def test_command_line_argument_errors(tmp_path, capsys):
    from panagram_amd.__main__ import main
    for argv, words in [(["pangenome"], "index_dir"),
                        (["pangenome", str(tmp_path / "nowhere")], "not an index directory"),
                        (["pangenome", str(tmp_path)], "config.yaml"),  # a directory that is no index
                        (["pangenome", str(tmp_path), "--matrix"], "--matrix"),
                        (["dist", "--exact"], "index_dir"),
                        (["index", "--kmer_stats"], "config_file")]:
        with pytest.raises(SystemExit) as ei:
            main(argv)
        assert ei.value.code == 2, argv
        assert words in capsys.readouterr().err, argv


def test_index_switch_is_a_flag_and_a_call_and_multi_process_runs_refuse(tmp_path):
    from panagram_amd import index as pidx
    fa = tmp_path / "a.fa"
    fa.write_text(">c\nACGTACGTACGTACGTACGTACGTACGTAC\n")
    (tmp_path / "samples.tsv").write_text(f"name\tfasta\na\t{fa}\nb\t{fa}\n")
    off = pidx.Index(str(tmp_path / "samples.tsv"), prefix=str(tmp_path / "i0"), k=K)
    on = pidx.Index(str(tmp_path / "samples.tsv"), prefix=str(tmp_path / "i1"), k=K, kmer_stats=True)
    assert not off.kmer_stats and on.kmer_stats and callable(on.kmer_stats) and callable(off.kmer_stats)
    assert "kmer_stats" not in on.params and on.params == {**off.params, "prefix": on.params["prefix"]}
    assert on.kmer_shared_fname.endswith("i1/kmer_shared.tsv") and on.kmer_occupancy_fname.endswith("i1/kmer_occupancy.tsv")
    for world in (2, 8):
        many = pidx.Index(str(tmp_path / "samples.tsv"), prefix=str(tmp_path / "i2"), k=K, kmer_stats=True, rank=0, world=world)
        with pytest.raises(ValueError, match="single-GPU"):
            many.run()
    # a cached table of some anchors' k-mers only cannot answer (no GPU needed to find that out)
    on._table, on._table_scope = object(), frozenset(["a"])
    with pytest.raises(RuntimeError, match=r"the cached table was built for the anchors \['a'\] only"):
        on.kmer_stats()
    with pytest.raises(RuntimeError, match="only"):
        on.write_genome_dist(exact=True)
    on._table, on._table_scope = None, "all"
