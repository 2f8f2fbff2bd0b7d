"""The numpy model of locate (tests/locate_ref.py) held to a brute-force dict search, every promise of its crafted case proved on
it, the host functions of panagram_amd/locate.py held to hand-written expectations, and the planted genomes of the end-to-end test
held to their truth.  No GPU."""
import numpy as np
import pandas as pd
import pytest

from panagram_amd import locate as loc
from tests import blocks_ref as br
from tests import locate_ref as lr

NO = lr.NO_MATE


def brute_hit_words(g, q, k):
    """the hit words by a dict of Q's windows as text: no packing, no canonical values, no sorting"""
    seen = {}
    off = 0
    for seq in q:
        s = bytes(seq).upper()
        for p in range(len(s) - k + 1):
            w = s[p:p + k]
            if set(w) <= set(b"ACGT"):
                r = lr.revcomp(w)
                seen.setdefault(min(w, r), []).append((off + p, int(w > r)))
        off += len(s)
    out = []
    for seq in g:
        s = bytes(seq).upper()
        for p in range(len(s) - k + 1):
            w = s[p:p + k]
            word = NO
            if set(w) <= set(b"ACGT"):
                r = lr.revcomp(w)
                found = seen.get(min(w, r), [])
                if len(found) == 1:
                    word = found[0][0] << 1 | (found[0][1] ^ int(w > r))
            out.append(word)
    return np.array(out, np.uint32)


def brute_runs(words, nk):
    out, off = [], 0
    for c, n in enumerate(nk):
        w = [int(x) for x in words[off:off + n]]
        off += n
        start = None
        for j in range(n + 1):
            cont = 0 < j < n and w[j] != NO and w[j - 1] != NO and w[j] - w[j - 1] == (-2 if w[j] & 1 else 2)
            if start is not None and not cont:
                out.append((c, start, j, w[start]))
                start = None
            if j < n and w[j] != NO and start is None:
                start = j
    return np.array(out, np.int64).reshape(-1, 4)


def random_case(seed, k, alphabet=b"ACGT"):
    rng = np.random.default_rng(seed)
    draw = lambda n: bytes(np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), n)])
    q = [draw(int(n)) for n in rng.integers(0, 60, 5)]
    g = [draw(int(n)) for n in rng.integers(0, 200, 3)]
    for i in range(3):  # copies of stretches of the queries, forward and reverse-complemented
        s = q[int(rng.integers(0, 5))]
        cut = s[int(rng.integers(0, max(1, len(s) // 2))):]
        g.append(draw(7) + (lr.revcomp(cut) if i & 1 else cut.lower()) + draw(5))
    return q, g


@pytest.mark.parametrize("k", [1, 2, 3, 6, 11, 21, 32])
def test_the_model_equals_a_dict_search(k):
    for seed, alphabet in ((k, b"ACGT"), (100 + k, b"ACGTNacgtn"), (200 + k, b"AC")):
        q, g = random_case(seed, k, alphabet)
        words, nk = lr.hit_words(g, q, k)
        assert nk == [max(0, len(s) - k + 1) for s in g]
        assert np.array_equal(words, brute_hit_words(g, q, k)), (k, seed)
        runs = lr.sr.runs(words, nk)
        assert np.array_equal(runs, brute_runs(words, nk)), (k, seed)
        if k >= 2:
            lr.hit_runs(g, q, k)  # (asserts that no run spans two queries)


def test_small_cases_against_the_dict_search():
    cases = lr.small_cases()
    for name, (k, q, g) in cases.items():
        words, nk = lr.hit_words(g, q, k)
        assert np.array_equal(words, brute_hit_words(g, q, k)), name
    # the palindrome at k = 6: one key, rc = 0 on both sides, so strand +; position 6 of query 0, position 300 of contig 0
    k, q, g = cases["k6"]
    words, nk = lr.hit_words(g, q, k)
    assert words[300] == 6 << 1
    # k = 31, 32: the forward copy, the reverse-complemented one, four positions of the lower-case one, the second forward copy of b
    for k in (31, 32):
        _, q, g = cases[f"k{k}"]
        runs, per, hits = lr.hit_runs(g, q, k)
        na, nb = 150 - k + 1, 90 - k + 1
        assert runs.tolist() == [[0, 70, 70 + na, 0], [0, 70 + 150 + 33, 70 + 150 + 33 + nb, (150 + nb - 1) << 1 | 1],
                                 [2, 0, 4, 10 << 1], [2, k + 4, k + 4 + nb, 150 << 1]]
        assert per.tolist() == [2, 0, 2] and hits.tolist() == [na + nb, 0, 4 + nb]
    k, q, g = cases["1025 queries"]
    runs, per, hits = lr.hit_runs(g, q, k)
    assert len(q) == 1025 and per.tolist() == [5, 1, 0]
    assert (runs[:, 3] >> 1).tolist() == [0, 511 * 40, 512 * 40, 1023 * 40, 1024 * 40, 700 * 40 + 19]
    assert lr.unique_per_query(q, k).tolist() == [20] * 1025
    # the eight key sets of a 64-slot table: every position of both queries is hit on both strands, two runs each
    for seed, (k, q, g) in enumerate(lr.wrap_cases()):
        words, nk = lr.hit_words(g, q, k)
        assert np.array_equal(words, brute_hit_words(g, q, k)), seed
        runs, per, hits = lr.hit_runs(g, q, k)
        assert per.tolist() == [2, 2] and hits.tolist() == [32, 32] and sorted(runs[:, 3] & 1) == [0, 0, 1, 1], seed


@pytest.fixture(scope="module")
def crafted():
    c = lr.crafted()
    c["words"], c["nk"] = lr.hit_words(c["g"], c["q"], c["k"])
    c["runs"], c["per"], c["hits"] = lr.hit_runs(c["g"], c["q"], c["k"])
    c["blocks"] = lr.blocks(c["g"], c["q"], c["k"], **c["params"])[0]
    c["qoff"] = np.concatenate([[0], np.cumsum([len(s) for s in c["q"]])])
    c["koff"] = np.concatenate([[0], np.cumsum(c["nk"])])
    return c


def _facts(p):
    return p if isinstance(p, list) else [p]


def test_crafted_has_the_shape_the_issue_asks_for(crafted):
    q, g, k = crafted["q"], crafted["g"], crafted["k"]
    assert k == 21 and len(q) == 39 and max(map(len, q)) == 9000 and min(len(s) for s in q if len(s) >= k) == 30
    assert 24_000 <= sum(map(len, g)) <= 28_000
    assert any(len(s) == 0 for s in q) and any(0 < len(s) < k for s in q)            # an empty Q contig, one shorter than k
    assert [len(s) for s in g[2:6]] == [20, 0, k, 3]                                 # contigs shorter than k between the others
    assert crafted["nk"][4] == 1


def test_every_promise_of_crafted_holds_on_the_model(crafted):
    words, runs, koff, qoff, k = crafted["words"], crafted["runs"], crafted["koff"], crafted["qoff"], crafted["k"]
    run_set = {tuple(r) for r in runs.tolist()}
    block_rows = crafted["blocks"].tolist()
    checked = 0
    for tag, p in crafted["promises"].items():
        if tag == "absent query":
            lo, hi = qoff[p], qoff[p + 1]
            hit = words[words != NO].astype(np.int64) >> 1
            assert not ((hit >= lo) & (hit < hi)).any(), tag
            continue
        for fact in _facts(p):
            checked += 1
            if fact[0] == "hits":
                _, c, at, n, qi, o, strand = fact
                first = (int(qoff[qi]) + o) << 1 | strand
                assert (c, at, at + n, first) in run_set, (tag, fact)
                got = words[koff[c] + at:koff[c] + at + n].astype(np.int64)
                assert np.array_equal(got, first + np.arange(n) * (-2 if strand else 2)), (tag, fact)
            elif fact[0] == "none":
                _, c, lo, hi = fact
                assert (words[koff[c] + lo:koff[c] + hi] == NO).all(), (tag, fact)
            else:
                _, c, start, end, qi, nruns, shifted = fact  # a locus in bases: [start, end) of contig c
                mine = [b for b in block_rows if b[0] == c and b[1] == start and b[2] + k - 1 == end]
                assert len(mine) == 1 and mine[0][6] == nruns and mine[0][7] == shifted, (tag, fact, mine)
                assert br.contig_of(mine[0][3] >> 1, [len(s) for s in crafted["q"]]) == qi
    assert checked >= 25


def test_crafted_holds_every_edge_of_the_kernel(crafted):
    runs, words, koff = crafted["runs"], crafted["words"], crafted["koff"]
    c, s, e = runs[:, 0], runs[:, 1], runs[:, 2]
    nk = np.asarray(crafted["nk"])[c]
    across = lambda step: ((s // step) != ((e - 1) // step))
    assert across(64).any() and across(256).any() and across(4096).any()             # runs over lane 63|64, 255|256, 4095|4096
    assert ((e - 1) // 4096 - s // 4096 >= 3).any()                                  # more than two whole chunks inside one run
    assert ((e % 4096 == 0) & (e < nk)).sum() >= 2                                   # ends exactly at a chunk's end
    starts = (s % 4096 == 0) & (s > 0)
    assert starts.sum() >= 2                                                         # starts exactly at a chunk's start ...
    before = words[koff[c[starts]] + s[starts] - 1]
    assert (before == NO).any() and (before != NO).any()                             # ... behind no hit, and behind a hit it does not continue
    # a position at a chunk's start that DOES continue its predecessor: the halo probe decides it
    w = words[koff[0]:koff[1]].astype(np.int64)
    assert w[4096] == w[4095] + 2 and w[8192] == w[8191] + 2
    assert (s == 0).any() and (e == nk).any() and ((s == 0) & (e == nk) & (nk == 1)).any()  # first, last, the only position
    # what the run scan decides from a neighbour that is not the lane below: a run whose last position is 4095 with the next one
    # starting at 4096 (end and start both from the halo), runs starting at a wave's and at a tile's first lane behind no hit, and
    # a run closed at the contig's end where the contig is a whole number of tiles, and where it is not
    at = {(int(ci), int(si)) for ci, si in zip(c, s)}
    assert any((int(ci), 4096) in at for ci, ei in zip(c, e) if ei == 4096)
    for first_lane in (64, 256):
        mine = s == first_lane
        assert mine.any() and (words[koff[c[mine]] + first_lane - 1] == NO).all(), first_lane
    assert crafted["nk"][7] <= 2 * 4096 + 300
    assert ((e == nk) & (nk % 256 == 0)).any() and ((e == nk) & (nk % 256 != 0) & (nk > 1)).any()
    assert (runs[:, 3] & 1).any()                                                    # a minus-strand run
    # pg_postable_mates would give the three copies nothing: their keys are not unique in G
    triple = crafted["promises"]["once in Q, three times in G"]
    assert len({tuple(words[koff[f[1]] + f[2]:koff[f[1]] + f[2] + f[3]]) for f in triple}) == 1
    assert crafted["per"].tolist() == np.bincount(c, minlength=len(crafted["g"])).tolist()
    assert crafted["hits"].sum() == (e - s).sum() == (words != NO).sum()


def test_unique_per_query(crafted):
    q, k, names = crafted["q"], crafted["k"], crafted["names"]
    u = lr.unique_per_query(q, k)
    kmers = np.array([max(0, len(s) - k + 1) for s in q])
    shared = 60 - k + 1  # the windows inside the stretch dup1 and dup2 share
    want = kmers.copy()
    want[names["dup1"]] -= shared
    want[names["dup2"]] -= shared
    assert u.tolist() == want.tolist() and u[names["empty"]] == 0 and u[names["short"]] == 0


# ---------------------------------------------------------------------------
# locate.py by hand
# ---------------------------------------------------------------------------
def _blocks(rows):
    a = np.array(rows, np.int64).reshape(-1, 8)
    return [a[:, i] for i in range(8)]


def hand_frames(**kw):
    k = 5
    qnames, qlens = ["q0", "q1", "q0", "tiny"], [30, 20, 12, 3]
    unique = [26, 10, 8, 0]
    # g0: chromosomes c0, c1; g1: chromosome z.  Blocks: contig, start, end, first word, last word, kmers, runs, shifted
    g0 = loc.genome_loci(_blocks([[0, 4, 30, 0 << 1, 25 << 1, 26, 1, 0],              # q0 whole, +
                                  [0, 100, 105, (30 + 9) << 1 | 1, (30 + 5) << 1 | 1, 5, 1, 0],   # q1 positions 9 down to 5, -
                                  [1, 7, 12, (50 + 2) << 1, (50 + 7) << 1, 5, 2, 1],  # the second q0: positions 2..7, one shifted link
                                  [1, 2, 4, 3 << 1, 4 << 1, 2, 1, 0]]), k, 2, qlens)  # q0, two k-mers (given unsorted on purpose: a frame sorts)
    g1 = loc.genome_loci(_blocks([[0, 0, 13, 12 << 1, 25 << 1, 13, 2, 0]]), k, 1, qlens)
    return loc.frames(qnames, qlens, k, unique, ["g0", "g1"], [(["c0", "c1"], g0), (["z"], g1)], **kw)


def test_frames_by_hand():
    loci, matrix, summary = hand_frames()
    assert list(loci.columns) == loc.LOCI_COLUMNS and list(summary.columns) == loc.SUMMARY_COLUMNS
    # sorted by query in file order, genome, chromosome in file order, start; half-open base ranges: end + k - 1, (last >> 1) + k
    assert loci.drop(columns=["frac"]).to_numpy().tolist() == [
        ["q0", "g0", "c0", 4, 34, "+", 0, 30, 26, 1, 0],
        ["q0", "g0", "c1", 2, 8, "+", 3, 9, 2, 1, 0],
        ["q0", "g1", "z", 0, 17, "+", 12, 30, 13, 2, 0],
        ["q1", "g0", "c0", 100, 109, "-", 5, 14, 5, 1, 0],
        ["q0", "g0", "c1", 7, 16, "+", 2, 12, 5, 2, 1]]
    assert loci["frac"].tolist() == [1.0, 2 / 26, 0.5, 0.5, 5 / 8]
    assert loci.attrs["qlen"] == [30, 30, 30, 20, 12]
    assert matrix.index.tolist() == ["q0", "q1", "q0", "tiny"] and matrix.columns.tolist() == ["g0", "g1"]
    assert matrix.to_numpy().tolist() == [[2, 1], [1, 0], [1, 0], [0, 0]]
    assert summary.to_numpy().tolist() == [["q0", 30, 26, 26, 3, 2, "g0", 1.0], ["q1", 20, 16, 10, 1, 1, "g0", 0.5],
                                           ["q0", 12, 8, 8, 1, 1, "g0", 5 / 8], ["tiny", 3, 0, 0, 0, 0, "-", 0.0]]


def test_frames_filters():
    loci, matrix, summary = hand_frames(min_kmers=5)
    assert loci["kmers"].tolist() == [26, 13, 5, 5] and matrix.to_numpy().tolist() == [[1, 1], [1, 0], [1, 0], [0, 0]]
    loci, matrix, summary = hand_frames(min_frac=0.5)  # (a frac of exactly min_frac stays)
    assert loci["frac"].tolist() == [1.0, 0.5, 0.5, 5 / 8]
    loci, matrix, summary = hand_frames(min_frac=0.6, min_kmers=6)
    assert loci[["query", "genome", "kmers"]].to_numpy().tolist() == [["q0", "g0", 26]]
    assert summary["loci"].tolist() == [1, 0, 0, 0] and summary["best_genome"].tolist() == ["g0", "-", "-", "-"]
    assert summary["unique"].tolist() == [26, 10, 8, 0]
    for bad in (dict(min_kmers=0), dict(min_frac=1.5), dict(min_frac=-0.1)):
        with pytest.raises(ValueError):
            hand_frames(**bad)


def test_frames_without_loci_or_queries():
    empty = loc.genome_loci(_blocks([]), 5, 0, [])
    loci, matrix, summary = loc.frames([], [], 5, [], ["g0"], [([], empty)])
    assert len(loci) == 0 and list(loci.columns) == loc.LOCI_COLUMNS and matrix.shape == (0, 1) and len(summary) == 0
    loci, matrix, summary = loc.frames(["a"], [9], 5, [5], [], [])
    assert len(loci) == 0 and matrix.shape == (1, 0) and summary.to_numpy().tolist() == [["a", 9, 5, 5, 0, 0, "-", 0.0]]
    with pytest.raises(ValueError, match="per genome"):
        loc.frames(["a"], [9], 5, [5], ["g0"], [])
    too_many = loc.genome_loci(_blocks([[0, 0, 6, 0, 10, 6, 1, 0]]), 5, 1, [10])
    with pytest.raises(ValueError, match="unique"):
        loc.frames(["a"], [10], 5, [5], ["g0"], [(["c"], too_many)])


def test_paf_lines_by_hand():
    loci = hand_frames()[0]
    lines = loc.paf_lines(loci, {"g0": {"c0": 500, "c1": 60}, "g1": {"z": 17}})
    assert lines == ["q0\t30\t0\t30\t+\tc0\t500\t4\t34\t26\t30\t255\trn:i:1\tsh:i:0\tgn:Z:g0",
                     "q0\t30\t3\t9\t+\tc1\t60\t2\t8\t2\t6\t255\trn:i:1\tsh:i:0\tgn:Z:g0",
                     "q0\t30\t12\t30\t+\tz\t17\t0\t17\t13\t18\t255\trn:i:2\tsh:i:0\tgn:Z:g1",
                     "q1\t20\t5\t14\t-\tc0\t500\t100\t109\t5\t9\t255\trn:i:1\tsh:i:0\tgn:Z:g0",
                     "q0\t12\t2\t12\t+\tc1\t60\t7\t16\t5\t10\t255\trn:i:2\tsh:i:1\tgn:Z:g0"]
    with pytest.raises(ValueError, match="attrs"):
        loc.paf_lines(pd.DataFrame(loci.to_dict("list")), {})


# ---------------------------------------------------------------------------
# the planted genomes of tests/test_gpu_locate_e2e.py
# ---------------------------------------------------------------------------
def test_planted_genomes_against_their_truth():
    genomes, genes, _, truth = lr.e2e_genomes()
    queries = lr.e2e_queries()
    k = lr.E2E_K
    for (gene, gname, chrom, s, e, strand, _) in truth:  # the truth is where the bytes are
        seq = genomes[lr.E2E_NAMES.index(gname)][lr.E2E_CHROMS.index(chrom)][s:e].upper()
        want = genes[gene][:e - s] if gene != "b" or gname == "g0" else seq
        assert seq == (lr.revcomp(want) if strand == "-" else want), (gene, gname)
    loci, matrix, summary = lr.loci_frames([n for n, _, _ in queries], [s for _, s, _ in queries],
                                           [(n, lr.E2E_CHROMS, g) for n, g in zip(lr.E2E_NAMES, genomes)], k)
    gene_of = [g for _, _, g in queries]
    qi = np.repeat(np.arange(len(queries)), matrix.to_numpy().sum(axis=1))  # (the loci are sorted by query)
    exact = set()
    for i, r in enumerate(loci.itertuples(index=False)):
        mine = [t for t in truth if t[0] == gene_of[qi[i]] and t[1] == r.genome and t[2] == r.chrom and t[3] <= r.start and r.end <= t[4]]
        assert len(mine) == 1 and mine[0][5] == r.strand, r  # every locus lies inside a planted copy of its query
        whole = summary["unique"].iloc[qi[i]] == summary["kmers"].iloc[qi[i]]
        if mine[0][6] and whole:  # a verbatim copy of a query whose k-mers are all unique: the planted interval exactly
            assert (r.start, r.end, r.qstart, r.qend, r.frac, r.runs) == (mine[0][3], mine[0][4], 0, len(queries[qi[i]][1]), 1.0, 1), r
            exact.add(mine[0])
    assert exact == {t for t in truth if t[6] and t[0] in "abcd"}
    assert matrix.to_numpy().tolist() == [[1, 3, 0], [1, 1, 0], [1, 0, 0], [0, 0, 0], [0, 0, 1], [1, 0, 0]]
    sub = loci[(loci["query"] == "geneB") & (loci["genome"] == "g1")].iloc[0]
    assert (sub["kmers"], sub["runs"], sub["shifted"]) == (880 - k, 2, 0)  # (the substitution takes the k windows over it)
    n = loci[loci["query"] == "withN"].iloc[0]
    assert (n["start"], n["end"], n["kmers"], n["runs"], n["frac"]) == (2113, 2713, 580 - k, 2, 1.0)
