"""The hit words, hit runs and loci of pg_locate.hip restated in numpy on tests/synteny_ref.py and tests/blocks_ref.py, and the
crafted queries and genome that hold every edge k_hit_runs has.  No tests in here: tests/test_locate_cpu.py ties the restatement to
a brute-force dict search and proves every promise of ``crafted()`` on it, tests/test_gpu_hit_runs.py and
tests/test_gpu_locate_e2e.py hold the kernel and the commands to it.

Q (the queries) and G (the streamed genome) are lists of contigs, each ASCII bytes.  The hit word of k-mer position p of a contig of
G is ``posQ << 1 | (rcG ^ rcQ)`` when the window is valid and its canonical key occurs exactly once among the valid windows of Q —
posQ global in Q's contigs laid end to end — and NO_MATE otherwise; G's own multiplicity does not matter.  A hit run is
``synteny_ref.runs`` of the hit words: positions of G are contig-relative."""
import numpy as np

from oracle import pyoracle as po
from tests import blocks_ref as br
from tests import synteny_ref as sr

NO_MATE = sr.NO_MATE
CHUNK, TILE, WAVE = 4096, 256, 64
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(s: bytes) -> bytes:
    return bytes(s).translate(_COMP)[::-1]


def hit_words(g, q, k):
    """(hit word of every k-mer position of G, contigs back to back [uint32]; k-mer positions per contig of G)"""
    kq, rcq, pq, _ = sr.side_kmers(q, k)
    uq, iq = sr.unique_of(kq)  # uniqueness is judged in Q only
    out, nk = [], []
    for seq in g:
        key, valid = po.canonical_kmers(bytes(seq), k)
        rc = (sr.forward_values(seq, k) > key).astype(np.int64)
        w = np.full(len(key), NO_MATE, np.int64)
        if len(uq) and len(key):
            j = np.minimum(np.searchsorted(uq, key), len(uq) - 1)
            hit = valid & (uq[j] == key)
            at = iq[j[hit]]
            w[hit] = (pq[at] << 1) | (rc[hit] ^ rcq[at])
        out.append(w)
        nk.append(len(key))
    return (np.concatenate(out) if out else np.zeros(0, np.int64)).astype(np.uint32), nk


def hit_runs(g, q, k):
    """(runs [n, 4] int64 = contig of G, start, end, hit word of the start; runs per contig; hit positions per contig)"""
    w, nk = hit_words(g, q, k)
    runs = sr.runs(w, nk)
    per = np.bincount(runs[:, 0], minlength=len(g)).astype(np.int64) if len(runs) else np.zeros(len(g), np.int64)
    offs = np.concatenate([[0], np.cumsum(nk)]).astype(np.int64)
    hits = np.array([int((w[offs[c]:offs[c + 1]] != NO_MATE).sum()) for c in range(len(g))], np.int64)
    if k >= 2:  # a run lies inside one query: neighbouring queries' k-mers lie at least k apart
        lens = [len(s) for s in q]
        for _, s, e, m in runs.tolist():
            assert br.contig_of(m >> 1, lens) == br.contig_of(br.last_mate(m, e - s) >> 1, lens), "a run spans two queries"
    return runs, per, hits


def unique_per_query(q, k):
    """the k-mer positions of every query whose k-mer occurs exactly once among the queries: Q streamed through its own table"""
    return hit_runs(q, q, k)[2]


def blocks(g, q, k, min_run=1, max_gap=1000, max_shift=100):
    """(blocks [n, 8] int64 — blocks_ref.COLUMNS, A = G and B = Q — , blocks per contig of G, hit positions, runs)"""
    runs, _, hits = hit_runs(g, q, k)
    blk = br.blocks(runs, [len(s) for s in q], min_run, max_gap, max_shift)
    per = np.bincount(blk[:, 0], minlength=len(g)).astype(np.int64) if len(blk) else np.zeros(len(g), np.int64)
    return blk, per, int(hits.sum()), len(runs)


def loci_frames(qnames, q, genomes, k, min_run=1, max_gap=1000, max_shift=100, min_kmers=1, min_frac=0.0):
    """``locate.frames`` of the model's arrays: ``genomes`` = [(name, chromosome names, contigs)].  Queries shorter than k take no
    part in the table, as in Index.locate."""
    from panagram_amd import locate as loc
    qlens = np.array([len(s) for s in q], np.int64)
    at = np.flatnonzero(qlens >= k)
    qk = [q[i] for i in at]
    unique = np.zeros(len(q), np.int64)
    if len(at):
        unique[at] = unique_per_query(qk, k)
    per = []
    for _, chroms, contigs in genomes:
        blk = blocks(contigs, qk, k, min_run, max_gap, max_shift)[0]
        f = loc.genome_loci([blk[:, i] for i in range(8)], k, len(contigs), qlens[at])
        f["chrB"] = at[f["chrB"].to_numpy(np.int64)]
        per.append((list(chroms), f))
    return loc.frames(list(qnames), qlens, k, unique, [n for n, _, _ in genomes], per, min_kmers, min_frac)


# ---------------------------------------------------------------------------
# the crafted queries and genome
# ---------------------------------------------------------------------------
def _rand(rng, n) -> bytes:
    return bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)])


class _Contig:
    """a contig of G: random bases with sequences written over them at chosen places, which do not touch"""

    def __init__(self, rng, n):
        self.b, self.taken = bytearray(_rand(rng, n)), []

    def put(self, at, seq):
        assert at >= 0 and at + len(seq) <= len(self.b)
        assert all(at >= e + 1 or at + len(seq) + 1 <= s for s, e in self.taken), "planted sequences touch"
        self.taken.append((at, at + len(seq)))
        self.b[at:at + len(seq)] = seq
        return at


CRAFTED_K = 21
CRAFTED_PARAMS = dict(min_run=1, max_gap=1000, max_shift=100)


def crafted():
    """dict(k, q, g, params, promises): about 40 queries of 30 to 9000 bases (an empty one, one shorter than k), a genome of a few
    contigs and 25 kb, and what they promise — name -> the facts tests/test_locate_cpu.py proves on the model:
      ("hits", c, p, n, qi, o, strand)   positions [p, p + n) of contig c of G are hits of positions o.. of query qi (descending from
                                         o on strand 1), and one run
      the others are spelled out in that test."""
    k = CRAFTED_K
    rng = np.random.default_rng(2024)
    q, name = [], {}

    def query(tag, seq):
        name[tag] = len(q)
        q.append(bytes(seq))
        return q[-1]
    first = query("first", _rand(rng, 50))
    lanes = query("lanes", _rand(rng, 120))
    tiles = query("tiles", _rand(rng, 100))
    long_ = query("long", _rand(rng, 9000))
    last = query("last", _rand(rng, 40))
    query("empty", b"")
    triple = query("triple", _rand(rng, 30))
    query("short", _rand(rng, 10))
    shared = _rand(rng, 60)
    dup1 = query("dup1", _rand(rng, 80) + shared + _rand(rng, 70))
    query("dup2", _rand(rng, 40) + shared + _rand(rng, 45))
    minus = query("minus", _rand(rng, 260))
    w = _rand(rng, k - 1)
    x, y = b"A", b"C"
    query("wy", _rand(rng, 90) + b"G" + w + y)   # ...Wy: the base in front of W is not x
    query("xw", x + w + b"T" + _rand(rng, 90))   # xW...: the base behind W is not y
    chunk_end = query("chunk_end", _rand(rng, 200))
    chunk_start = query("chunk_start", _rand(rng, 150))
    after_n = query("after_n", _rand(rng, 90))
    lower = query("lower", _rand(rng, 130))
    tandem = query("tandem", _rand(rng, 180))
    sub = query("sub", _rand(rng, 300))
    ins = query("ins", _rand(rng, 300))
    dele = query("del", _rand(rng, 300))
    query("absent", _rand(rng, 500))
    single = query("single", _rand(rng, 64))
    for i in range(16):  # bystanders, of which G holds every fourth (contig 6) and the first three others (contig 7)
        query(f"extra{i}", _rand(rng, 30 + 61 * i))
    promises = {}

    # contig 0: 13000 bases.  A hit at its first position; runs across 127|128 (lane 63|64 of a wave) and 255|256; the long query
    # from 3500 on: one run over 4095|4096 that covers the chunks [4096, 8192) and [8192, 12288) whole; a hit at its last position
    c0 = _Contig(rng, 13000)
    c0.put(0, first)
    c0.put(100, lanes)
    c0.put(230, tiles)
    c0.put(3500, long_)
    c0.put(13000 - len(last), last)
    promises["first position"] = ("hits", 0, 0, 50 - k + 1, name["first"], 0, 0)
    promises["lane 63|64"] = ("hits", 0, 100, 120 - k + 1, name["lanes"], 0, 0)
    promises["255|256"] = ("hits", 0, 230, 100 - k + 1, name["tiles"], 0, 0)
    promises["two whole chunks"] = ("hits", 0, 3500, 9000 - k + 1, name["long"], 0, 0)
    promises["last position"] = ("hits", 0, 13000 - 40, 40 - k + 1, name["last"], 0, 0)

    # contig 1: 9000 bases.  One key three times; the shared stretch of dup1 / dup2 (no hit inside); a minus-strand run; xWy with
    # Wy at position 4096: a run that ends at a chunk's end against a hit that does not continue it; a run that ends at 8192
    # against no hit; an N directly in front of a hit; lower case
    c1 = _Contig(rng, 9000)
    for at in (100, 300, 500):
        c1.put(at, triple)
    promises["once in Q, three times in G"] = [("hits", 1, at, 30 - k + 1, name["triple"], 0, 0) for at in (100, 300, 500)]
    c1.put(700, dup1)
    # (a window that holds a base of dup1's own flanks is dup1's alone: only the 40 windows inside the shared stretch repeat)
    promises["twice in Q"] = [("hits", 1, 700, 80, name["dup1"], 0, 0), ("none", 1, 780, 820), ("hits", 1, 820, 70, name["dup1"], 120, 0)]
    c1.put(1000, revcomp(minus))
    promises["minus strand"] = ("hits", 1, 1000, 260 - k + 1, name["minus"], 260 - k, 1)
    c1.put(4095, x + w + y)
    promises["neighbours, not collinear"] = [("hits", 1, 4095, 1, name["xw"], 0, 0), ("hits", 1, 4096, 1, name["wy"], 91, 0)]
    c1.put(8192 - (200 - k + 1), chunk_end)
    promises["ends at a chunk's end"] = ("hits", 1, 8192 - 180, 180, name["chunk_end"], 0, 0)
    c1.put(2000, b"N" + after_n)
    promises["N in front of a hit"] = [("none", 1, 2000 - k + 1, 2001), ("hits", 1, 2001, 90 - k + 1, name["after_n"], 0, 0)]
    c1.put(2300, lower.lower())
    promises["lower case"] = ("hits", 1, 2300, 130 - k + 1, name["lower"], 0, 0)
    promises["absent key"] = ("none", 1, 5000, 6000)

    # contigs 2 to 5: shorter than k, empty, exactly k bases that are a hit, shorter than k
    small = [_rand(rng, 20), b"", single[30:30 + k], _rand(rng, 3)]
    promises["one position"] = ("hits", 4, 0, 1, name["single"], 30, 0)

    # contig 6: 4400 bases.  A tandem duplicate; a copy with a substitution, one with three bases more, one with five fewer; a run
    # from position 4096 on, behind no hit; every fourth bystander
    c6 = _Contig(rng, 4400)
    c6.put(50, tandem + tandem)
    promises["tandem"] = [("locus", 6, 50, 50 + 180, name["tandem"], 1, 0), ("locus", 6, 50 + 180, 50 + 360, name["tandem"], 1, 0)]
    s = bytearray(sub)
    s[150] = b"ACGT"[(b"ACGT".index(s[150]) + 1) & 3]
    c6.put(500, bytes(s))
    promises["substitution"] = ("locus", 6, 500, 800, name["sub"], 2, 0)
    more = bytes([b"ACGT"[(b"ACGT".index(ins[150]) + 1) & 3]]) + b"A" + bytes([b"ACGT"[(b"ACGT".index(ins[149]) + 1) & 3]])
    c6.put(900, ins[:150] + more + ins[150:])
    promises["insertion"] = ("locus", 6, 900, 1203, name["ins"], 2, 1)
    d = bytearray(dele)
    d[149], d[150], d[154], d[155] = b"GATC"  # (no match runs on across the deletion)
    q[name["del"]] = dele = bytes(d)
    c6.put(1300, dele[:150] + dele[155:])
    promises["deletion"] = ("locus", 6, 1300, 1595, name["del"], 2, 1)
    at = 1700
    for i in range(0, 16, 4):
        c6.put(at, q[name[f"extra{i}"]])
        at += len(q[name[f"extra{i}"]]) + 40
    c6.put(4096, chunk_start)
    promises["starts at a chunk's start"] = [("none", 6, 4096 - k, 4096), ("hits", 6, 4096, 150 - k + 1, name["chunk_start"], 0, 0)]
    promises["absent query"] = name["absent"]

    # contig 7: 768 k-mer positions, three tiles exactly.  Three more bystanders: a run that STARTS at position 64 (its predecessor
    # is the wave's below), one that starts at 256 (the tile's before), one that reaches the contig's end at a tile's end
    c7 = _Contig(rng, 3 * TILE + k - 1)
    for tag, at, i in (("starts at a wave's start", WAVE, 1), ("starts at a tile's start", TILE, 2), ("ends with the last tile", None, 3)):
        seq = q[name[f"extra{i}"]]
        at = c7.put(len(c7.b) - len(seq) if at is None else at, seq)
        promises[tag] = [("none", 7, at - 1, at), ("hits", 7, at, len(seq) - k + 1, name[f"extra{i}"], 0, 0)]
    g = [bytes(c0.b), bytes(c1.b)] + small + [bytes(c6.b), bytes(c7.b)]
    return dict(k=k, q=q, g=g, params=dict(CRAFTED_PARAMS), promises=promises, names=name)


def small_cases():
    """name -> (k, q, g): k = 6 with a reverse-complement palindrome and keys that repeat everywhere, k = 31 and k = 32 with a
    forward, a reverse-complemented and a lower-case copy, and 1025 queries of 40 bases"""
    rng = np.random.default_rng(77)
    cases = {}
    pal = b"ACGCGT"  # its own reverse complement
    q6 = [b"TTTTTT" + pal + b"TTTTT", _rand(rng, 40), _rand(rng, 25)]
    cases["k6"] = (6, q6, [_rand(rng, 300) + pal + _rand(rng, 290), q6[1][5:30] + b"N" + revcomp(q6[2])])
    for k in (31, 32):
        a, b = _rand(rng, 150), _rand(rng, 90)
        cases[f"k{k}"] = (k, [a, b, _rand(rng, k - 1)],
                          [_rand(rng, 70) + a + _rand(rng, 33) + revcomp(b) + _rand(rng, 5), b"", a.lower()[10:10 + k + 3] + b"n" + b])
    many = [_rand(rng, 40) for _ in range(1025)]
    held = [many[i] for i in (0, 511, 512, 1023, 1024)]
    cases["1025 queries"] = (21, many, [b"".join(s + _rand(rng, 7) for s in held), revcomp(many[700]), _rand(rng, 20)])
    return cases


def wrap_cases():
    """eight (k, q, g): two queries of 12 and 20 k-mer positions, 32 distinct keys — a table made for them has 64 slots and is half
    full, and over eight key sets a key whose home is one of the last slots walks on at slot 0.  The genome holds each query forward
    and reverse-complemented between random flanks."""
    k, cases = 21, []
    for seed in range(8):
        rng = np.random.default_rng(100 + seed)
        q = [_rand(rng, 12 + k - 1), _rand(rng, 20 + k - 1)]
        g = [_rand(rng, 50) + q[0] + _rand(rng, 31) + revcomp(q[1]) + _rand(rng, 40), _rand(rng, 9) + revcomp(q[0]) + _rand(rng, 64) + q[1]]
        assert unique_per_query(q, k).tolist() == [12, 20]  # (every position's key is held once: 32 distinct keys)
        cases.append((k, q, g))
    return cases


# ---------------------------------------------------------------------------
# three small genomes with planted genes, shared by tests/test_locate_cpu.py and tests/test_gpu_locate_e2e.py
# ---------------------------------------------------------------------------
E2E_K = 21
E2E_NAMES = ["g0", "g1", "g2"]
E2E_CHROMS = ["chr1", "chr2"]


def e2e_genomes():
    """(per genome its two chromosomes; the genes by name; the genes of g0's GFF as (chromosome, start, end); the truth: per
    planted copy (gene, genome, chromosome, start, end, strand, verbatim)).  A once in g0 and three times in g1 (forward,
    reverse-complemented, lower case); B once in g0 and with one substitution in g1; C in g0 only; D in g2 only; f1, the stretch
    between A and B in g0, is what the query with an N is cut from."""
    rng = np.random.default_rng(41)
    a, b, c, d = _rand(rng, 1500), _rand(rng, 900), _rand(rng, 400), _rand(rng, 350)
    f = [_rand(rng, 700) for _ in range(8)]
    b_sub = bytearray(b)
    b_sub[300] = b"ACGT"[(b"ACGT".index(b_sub[300]) + 1) % 4]
    g0 = [f[0][:613] + a + f[1] + b + f[2], f[3][:77] + c + f[4]]
    g1 = [f[5] + a + f[6] + revcomp(a) + f[0] + a.lower(), bytes(b_sub) + f[7]]
    g2 = [_rand(rng, 3000) + b"NNNNN" + _rand(rng, 500).lower(), _rand(rng, 200) + d + _rand(rng, 450)]
    genes = [("chr1", 613, 2113), ("chr1", 2813, 3713), ("chr2", 77, 477), ("chrZ", 10, 500), ("chr1", 900, 880), ("chr2", 1100, 5000)]
    truth = [("a", "g0", "chr1", 613, 2113, "+", True), ("a", "g1", "chr1", 700, 2200, "+", True), ("a", "g1", "chr1", 2900, 4400, "-", True),
             ("a", "g1", "chr1", 5100, 6600, "+", True), ("b", "g0", "chr1", 2813, 3713, "+", True), ("b", "g1", "chr2", 0, 900, "+", False),
             ("c", "g0", "chr2", 77, 477, "+", True), ("d", "g2", "chr2", 200, 550, "+", True), ("f1", "g0", "chr1", 2113, 2713, "+", False),
             ("f0", "g0", "chr1", 0, 613, "+", False), ("f0", "g1", "chr1", 4400, 5100, "+", False)]
    return [g0, g1, g2], dict(a=a, b=b, c=c, d=d, f1=f[1], f0=f[0]), genes, truth


def e2e_queries():
    """[(name, sequence, gene)], in file order: a duplicate name (another sequence), a query shorter than k, one with an N"""
    g = e2e_genomes()[1]
    return [("geneA", g["a"], "a"), ("geneB", g["b"], "b"), ("geneC", g["c"], "c"), ("short", g["a"][:E2E_K - 1], None), ("geneA", g["d"], "d"),
            ("withN", g["f1"][:300] + b"N" + g["f1"][301:600], "f1")]
