"""CPU: tests/copies_ref.py — the numpy model the copy-number kernels are held to — on genomes whose depths follow by construction.

A random genome gets a 3 kb "gene" planted once, twice (the second copy reverse-complemented), as a tandem array of five, once more
with two substitutions, and into a second contig.  Exact values are asserted only behind ``clean``: the test itself shows, for its
seed, that the gene repeats no k-mer and shares none with the random flanks."""
import numpy as np
import pytest

from tests import copies_ref as cr

K = 21
GENE = 3000
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def rand(rng, n):
    return bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)])


def revcomp(s):
    return s.translate(_COMP)[::-1]


def substituted(s, sites):
    b = bytearray(s)
    for i in sites:
        b[i] = b"ACGT"[(b"ACGT".index(b[i]) + 1) % 4]
    return bytes(b)


@pytest.fixture(scope="module")
def planted():
    rng = np.random.default_rng(20)
    gene = rand(rng, GENE)
    f = [rand(rng, 4000) for _ in range(12)]
    far, near = (700, 1900), (1200, 1200 + K - 1)  # two substitutions k or more apart, and k - 1 apart
    genomes = {
        "once": [f[0] + gene + f[1]],
        "twice": [f[0] + gene + f[1] + revcomp(gene) + f[2]],
        "tandem": [f[0] + gene * 5 + f[1]],
        "sub_far": [f[0] + gene + f[1] + substituted(gene, far) + f[2]],
        "sub_near": [f[0] + gene + f[1] + substituted(gene, near) + f[2]],
        "second": [f[0] + gene + f[1], f[2] + gene + f[3]],
        "none": [f[0] + f[1]],
    }
    genomes["all"] = [b"".join(c for name in ("once", "twice", "tandem", "sub_far") for c in genomes[name]), genomes["second"][1]]
    gk = cr.valid_keys([gene], K)
    clean = len(np.unique(gk)) == len(gk) and not np.isin(cr.valid_keys(f, K), gk).any()
    # (the substituted windows must be new k-mers too: not in the gene, not in the flanks)
    for sites in (far, near):
        sk = cr.valid_keys([substituted(gene, sites)], K)
        new = sk[~np.isin(sk, gk)]
        clean = clean and not np.isin(new, cr.valid_keys(f, K)).any() and len(np.unique(new)) == len(new)
    return dict(gene=gene, genomes=genomes, clean=bool(clean), far=far, near=near)


def median_of(hist):
    cum = np.cumsum(hist.astype(np.int64))
    return int((2 * cum >= cum[-1]).argmax())


def test_the_seed_is_clean(planted):
    assert planted["clean"]


def test_medians_follow_the_planting(planted):
    assert planted["clean"]
    names = ["none", "once", "twice", "tandem", "sub_far", "sub_near", "second", "all"]
    hist, valid, track = cr.profile([planted["gene"]], [planted["genomes"][n] for n in names], K)
    n = GENE - K + 1
    assert valid.tolist() == [n]
    assert (hist.sum(axis=2) == valid[:, None]).all()
    med = {name: median_of(hist[0, i]) for i, name in enumerate(names)}
    assert med == dict(none=0, once=1, twice=2, tandem=5, sub_far=2, sub_near=2, second=2, all=11)
    # every position of the gene has the planted depth, but the substituted windows
    for name, d in (("none", 0), ("once", 1), ("twice", 2), ("tandem", 5), ("second", 2)):
        assert hist[0, names.index(name), d] == n and (track[names.index(name)] == d).all()


def test_substitutions_lower_exactly_the_windows_over_them(planted):
    assert planted["clean"]
    g = planted["genomes"]
    hist, valid, track = cr.profile([planted["gene"]], [g["sub_far"], g["sub_near"], g["all"]], K)
    n = GENE - K + 1
    for row, sites, lowered in ((0, planted["far"], 2 * K), (1, planted["near"], 2 * K - 1)):
        want = np.full(n, 2)
        for s in sites:
            want[max(0, s - K + 1):s + 1] = 1  # the windows that hold base s
        assert (track[row] == want).all()
        assert hist[0, row, 1] == lowered and hist[0, row, 2] == n - lowered
    # in the genome that holds every form, 1 + 2 + 5 + 2 and 1 in its second contig: the substituted copy lowers 2k windows by one
    assert hist[0, 2, 11] == n - 2 * K and hist[0, 2, 10] == 2 * K


def test_targets_are_not_deduplicated(planted):
    gene, g = planted["gene"], planted["genomes"]["tandem"]
    hist, valid, track = cr.profile([gene, gene[500:1500], gene + gene], [g], K)
    assert valid.tolist() == [GENE - K + 1, 1000 - K + 1, 2 * GENE - K + 1]
    assert hist[1, 0, 5] == valid[1]
    # the doubled target: its junction k-mers are the tandem array's own, four of them in five copies
    assert hist[2, 0, 5] == 2 * (GENE - K + 1) and hist[2, 0, 4] == K - 1


def test_n_and_lower_case():
    rng = np.random.default_rng(3)
    gene = rand(rng, 400)
    genome = [rand(rng, 1000) + gene + rand(rng, 1000)]
    with_n = gene[:100] + b"N" + gene[101:]
    hist, valid, track = cr.profile([gene, gene.lower(), with_n, with_n.lower().replace(b"n", b"x")], [genome], K)
    n = 400 - K + 1
    assert valid.tolist() == [n, n, n - K, n - K]
    assert (hist[0] == hist[1]).all() and (hist[2] == hist[3]).all()
    at = np.concatenate([[0], np.cumsum([n, n, n, n])])
    t2 = track[0, at[2]:at[3]]
    assert (t2[100 - K + 1:101] == cr.DEPTH_INVALID).all() and (t2 != cr.DEPTH_INVALID).sum() == n - K
    # an N in the genome: the windows over it do not exist, the depth drops to 0 there
    cut = [genome[0][:1000 + 200] + b"N" + genome[0][1000 + 201:]]
    d, v = cr.depths([gene], cut, K)[0]
    assert v.all() and (d[200 - K + 1:201] == 0).all() and (np.delete(d, np.arange(200 - K + 1, 201)) >= 1).all()
    assert cr.hits([gene], cut, K) == int(d.sum())


def test_short_targets():
    rng = np.random.default_rng(4)
    genome = [rand(rng, 3000)]
    exact = genome[0][100:100 + K]
    hist, valid, track = cr.profile([exact[:K - 1], exact, b"", revcomp(exact)], [genome], K)
    assert valid.tolist() == [0, 1, 0, 1]
    assert hist[0].sum() == 0 and hist[2].sum() == 0
    assert track.shape == (1, 2) and (track >= 1).all() and (track < cr.DEPTH_INVALID).all()
    assert hist[1, 0, int(track[0, 0])] == 1 and hist[3, 0, int(track[0, 1])] == 1


def test_homopolymer_lands_in_the_last_bin():
    rng = np.random.default_rng(5)
    genome = [rand(rng, 2000) + b"A" * 5000 + rand(rng, 2000), b"ACGT" * 3]  # (the second contig is shorter than k)
    hist, valid, track = cr.profile([b"A" * 100, b"T" * 100], [genome], K)
    assert valid.tolist() == [100 - K + 1] * 2
    assert (hist[:, 0, cr.BINS - 1] == 100 - K + 1).all() and hist[:, 0, :cr.BINS - 1].sum() == 0
    depth = 5000 - K + 1
    assert set(track[0].tolist()) <= {depth, depth + 1, depth + 2} and int(track[0, 0]) >= depth  # (a stray A-run in the flanks adds at most a few)
    assert cr.hits([b"A" * 100], genome, K) == int(track[0, 0])
    assert cr.distinct([b"A" * 100, b"T" * 100], K) == 1
