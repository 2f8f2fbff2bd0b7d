"""What pg_genotype.hip computes and what panagram_amd/genotype.py makes of it, restated the obvious way: a count table as a set of
canonical keys with one dict of counts per plane (tests/copies_ref.py's keys_of / valid_keys), the windows of an allele range by a
plain loop, the piece cutter, the call rule and the frames as loops over sites.  No tests in here: tests/test_genotype_cpu.py ties
the restatement to a planted sample whose genotypes follow by construction, tests/test_gpu_allele_support.py and
tests/test_gpu_genotype_e2e.py hold the kernels and the command to it.

Definitions (the header of panagram_amd/csrc/pg_genotype.hip in the same words), k the table's k:
  allele range    (c, s, l): bases [s, s + l) of contig c of a sequence set, s + l <= the contig's length L; l = 0 is the junction
                  between base s - 1 and base s.
  allele windows  the k-mer positions p of contig c with max(0, s - k + 1) <= p < min(L - k + 1, s + l).  For l = 0 the k - 1
                  windows that hold both neighbours of the junction; none when L < k; none for a junction at s = 0 or s = L; a
                  window holding a non-ACGT base does not exist.
  informative     an allele window with canonical key K is informative when own[K] == 1 and other[K] == 0; it is seen when also
                  sample[K] >= min_count.  A key the table does not hold reads 0 in all three planes.
  per range       windows = the allele windows that exist, inf = the informative ones, seen = the seen ones, depth = the sum of
                  sample[K] over the informative ones.
  call rule       an allele is present when inf > 0 and seen >= F * inf.  GT is ./. (flag uninformative) when either side has
                  inf == 0; otherwise 0/1 when both are present, 0/0 when only ref, 1/1 when only alt, ./. (flag neither) when
                  neither."""
import numpy as np

from oracle import pyoracle as po
from tests import copies_ref as cr
from tests import synteny_ref as sr
from tests import variants_ref as vr

PIECE = 64
CLASSES = ("same", "snp", "mnp", "ins", "del", "complex")
TABLE_COLUMNS = ["chrA", "posA", "refLen", "chrB", "posB", "altLen", "strand", "class", "ref", "alt", "ref_kmers", "ref_seen", "ref_depth",
                 "alt_kmers", "alt_seen", "alt_depth", "GT", "flag"]
GENOTYPES = ("0/0", "0/1", "1/1", "./.")


# ---------------------------------------------------------------------------
# windows, pieces, the table
# ---------------------------------------------------------------------------
def window_interval(L, k, s, l):
    """[p0, p1) of the allele windows of bases [s, s + l) of a contig of L bases, valid or not; p0 == p1: none"""
    assert 0 <= s and 0 <= l and s + l <= L
    p0, p1 = max(0, s - k + 1), min(L - k + 1, s + l)
    return (p0, p1) if p1 > p0 else (p0, p0)


def cut(p0, p1):
    """the pieces (first window, windows) of [p0, p1), at most PIECE windows each, in order"""
    out = []
    while p0 < p1:
        n = min(PIECE, p1 - p0)
        out.append((p0, n))
        p0 += n
    return out


def counts_of(contigs, k, weights=None):
    """canonical key -> how many valid windows of the contigs hold it; ``weights``: per contig, one count per k-mer position (how
    many times that window is read) in place of 1"""
    ks = cr.keys_of(contigs, k)
    if weights is None:
        u, n = np.unique(cr.valid_keys(contigs, k), return_counts=True)
        return dict(zip(u.tolist(), n.tolist()))
    out = {}
    for (key, valid), w in zip(ks, weights):
        w = np.asarray(w, np.int64)[:len(key)]
        u, inv = np.unique(key[valid], return_inverse=True)
        for a, b in zip(u.tolist(), np.bincount(inv, weights=w[valid], minlength=len(u)).astype(np.int64).tolist()):
            if b:
                out[a] = out.get(a, 0) + b
    return out


class Table:
    """the count table: the keys inserted, and per plane key -> count of the keys it held when the plane was counted"""

    def __init__(self, k, nplanes):
        self.k, self.keys, self.planes, self._kv = k, set(), [dict() for _ in range(nplanes)], None

    def _keys(self, contigs, ranges):
        """per range the canonical keys of its allele windows that exist, in position order"""
        if self._kv is None or self._kv[0] is not contigs:
            self._kv = (contigs, cr.keys_of(contigs, self.k))  # (the same set asked again: its keys are kept)
        out = []
        for c, s, l in ranges:
            key, valid = self._kv[1][c]
            p0, p1 = window_interval(len(contigs[c]), self.k, s, l)
            out.append([int(key[p]) for p in range(p0, p1) if valid[p]])
        return out

    def insert_ranges(self, contigs, ranges) -> int:
        """the keys newly added"""
        before = len(self.keys)
        for keys in self._keys(contigs, ranges):
            self.keys.update(keys)
        return len(self.keys) - before

    def count(self, plane, counts) -> int:
        """``counts`` (counts_of a genome or a read set) added to the plane for the keys the table holds; the hits"""
        hits = 0
        for key, n in counts.items():
            if key in self.keys:
                self.planes[plane][key] = self.planes[plane].get(key, 0) + n
                hits += n
        return hits

    def support(self, contigs, ranges, own, other, sample, min_count):
        """(windows, inf, seen, depth), one int per range"""
        po_, pt, ps = self.planes[own], self.planes[other], self.planes[sample]
        out = [[], [], [], []]
        for keys in self._keys(contigs, ranges):
            inf = [x for x in keys if x in self.keys and po_.get(x, 0) == 1 and pt.get(x, 0) == 0]
            out[0].append(len(keys))
            out[1].append(len(inf))
            out[2].append(sum(1 for x in inf if ps.get(x, 0) >= min_count))
            out[3].append(sum(ps.get(x, 0) for x in inf))
        return tuple(out)


# ---------------------------------------------------------------------------
# the call rule and the frames
# ---------------------------------------------------------------------------
def present(inf, seen, min_frac):
    return inf > 0 and seen >= min_frac * inf


def call(ref_inf, ref_seen, alt_inf, alt_seen, min_frac):
    """(GT, flag) of one site"""
    if ref_inf == 0 or alt_inf == 0:
        return "./.", "uninformative"
    r, a = present(ref_inf, ref_seen, min_frac), present(alt_inf, alt_seen, min_frac)
    if r and a:
        return "0/1", ""
    if r:
        return "0/0", ""
    if a:
        return "1/1", ""
    return "./.", "neither"


def mean_depth(depth, inf):
    return "." if inf == 0 else f"{depth / inf:.2f}"


def table_rows(sites, ref_support, alt_support, min_frac):
    """one list of TABLE_COLUMNS' values per site; sites: (chrA, posA, refLen, chrB, posB, altLen, strand, class, ref, alt)"""
    rows = []
    for i, site in enumerate(sites):
        (_, ri, rs, rd), (_, ai, as_, ad) = ([int(x[i]) for x in side] for side in (ref_support, alt_support))
        gt, flag = call(ri, rs, ai, as_, min_frac)
        rows.append(list(site) + [ri, rs, mean_depth(rd, ri), ai, as_, mean_depth(ad, ai), gt, flag])
    return rows


def table_text(rows):
    """the table as the command prints it"""
    lines = ["\t".join(TABLE_COLUMNS)]
    for r in rows:
        r = list(r)
        for i in (8, 9, 17):
            r[i] = r[i] or "-"
        lines.append("\t".join(str(v) for v in r))
    return "\n".join(lines) + "\n"


def summary_text(rows, reads, hits, ref_support, alt_support, min_count, min_frac):
    windows = sum(int(x) for x in ref_support[0]) + sum(int(x) for x in alt_support[0])
    lines = [f"# reads\t{reads}", f"# windows\t{windows}", f"# hits\t{hits}", f"# sites\t{len(rows)}",
             f"# callable\t{sum(1 for r in rows if r[17] != 'uninformative')}", f"# min_count\t{min_count}", f"# min_frac\t{min_frac:.6f}",
             "class\tGT\tcount"]
    for cls in CLASSES[1:]:
        for g in GENOTYPES:
            n = sum(1 for r in rows if r[7] == cls and r[16] == g)
            if n:
                lines.append(f"{cls}\t{g}\t{n}")
    return "\n".join(lines) + "\n"


def vcf_body(rows, anchors):
    """the VCF lines below the header, fields CHROM POS REF ALT FORMAT sample: the snp / mnp at posA + 1, the others behind their anchor base"""
    out = []
    for r, base in zip(rows, anchors):
        pos, ref, alt = (r[1] + 1, r[8], r[9]) if r[7] in ("snp", "mnp") else (r[1], base + r[8], base + r[9])
        out.append((r[0], str(pos), ref, alt, "GT:RK:AK", f"{r[16]}:{r[11]},{r[10]}:{r[14]},{r[13]}"))
    return out


# ---------------------------------------------------------------------------
# the crafted set of tests/test_gpu_allele_support.py
# ---------------------------------------------------------------------------
MIN_COUNT = 3
LONG_RUN = 70000  # a homopolymer whose one key the sample holds more than 65 535 times


def calm(codes, run=5):
    """random codes with every run of ``run`` equal bases broken: no homopolymer k-mer, k >= 6, by chance"""
    out = np.array(codes, np.uint8)
    same = 1
    for i in range(1, len(out)):
        same = same + 1 if out[i] == out[i - 1] else 1
        if same >= run:
            out[i] = (out[i] + 1 + (i & 1)) & 3
            same = 1
    return out


def _rand(n, seed):
    return sr.ascii_of(calm(sr.random_codes(n, seed)))


def crafted(k):
    """dict: ``seqs`` the contigs the ranges lie on; ``genomes`` [own, other, sample] as lists of contigs; ``inserted`` two range
    lists for two successive inserts; ``ranges`` name -> (contig, start, len), every one of them asked for in one support call —
    ``never`` is not inserted"""
    c0 = _rand(6000, 101)
    withn = bytearray(_rand(200, 102))
    withn[100] = ord("N")
    seqs = [c0, _rand(k - 1, 103), _rand(k, 104), bytes(withn), b"A" * LONG_RUN, _rand(300, 105), _rand(300, 106)]
    L = len(c0)
    r = {"one_base": (0, 500, 1), "junction": (0, 600, 0), "junction_at_0": (0, 0, 0), "junction_at_L": (0, L, 0),
         "first_window": (0, 2, 3), "last_window": (0, L - 2, 2), "first_base": (0, 0, 1), "last_base": (0, L - 1, 1),
         "short_contig": (1, 0, k - 1), "short_junction": (1, 1, 0), "exact_contig": (2, 0, k), "exact_junction": (2, 3, 0),
         "n_inside": (3, 95, 10), "n_beside": (3, 100 - (k - 1), 1), "n_alone": (3, 100, 1),
         "shares_a": (0, 500, 1), "shares_b": (0, 503, 2),
         # (every window of these two lies inside the 100 bases that own holds twice / other holds too)
         "twice_in_own": (0, 1000 + k - 1, 102 - 2 * k), "own_and_other": (0, 2000 + k - 1, 102 - 2 * k), "in_neither": (5, 50, 100), "never": (6, 50, 100),
         "depth_0": (0, 5000, 30), "depth_below": (0, 3500, 30), "depth_at": (0, 100, 30), "depth_across": (0, 2990, 20),
         "long_run": (4, 0, LONG_RUN), "long_run_junction": (4, 1000, 0)}
    for w in (63, 64, 65, 257, 4097):
        r[f"windows_{w}"] = (0, 700, w - k + 1)
    own = [c0, c0[1000:1100], b"C" + b"A" * k + b"G", seqs[6], seqs[2], bytes(withn)]
    other = [c0[2000:2100], _rand(500, 107)]
    sample = [c0[:3000]] * MIN_COUNT + [c0[3000:4500]] * (MIN_COUNT - 1) + [b"A" * LONG_RUN, seqs[2], bytes(withn)]
    names = [n for n in r if n != "never"]
    first = [r[n] for n in names[::2]]
    second = [r[n] for n in names[1::2]] + [r[names[0]]]
    return dict(seqs=seqs, genomes=[own, other, sample], inserted=[first, second], ranges=r)


def crafted_model(case, k):
    """(Table after both inserts and the three counts, [distinct of insert 1, of insert 2], [hits per plane])"""
    t = Table(k, 3)
    distinct = [t.insert_ranges(case["seqs"], rs) for rs in case["inserted"]]
    hits = [t.count(g, counts_of(case["genomes"][g], k)) for g in range(3)]
    return t, distinct, hits


def many_ranges(n=3000, seed=7):
    """n ranges on contig 0 of ``crafted``: (contig, start, len), lengths 0 to 40"""
    rng = np.random.default_rng(seed)
    return [(0, int(s), int(l)) for s, l in zip(rng.integers(0, 5900, n), rng.integers(0, 41, n))]


# ---------------------------------------------------------------------------
# the planted genomes and read sets of tests/test_genotype_cpu.py and tests/test_gpu_genotype_e2e.py
# ---------------------------------------------------------------------------
E2E_CHROMS = ["chr1", "chr2", "chr3"]
E2E_LENS = (20000, 15000, 9000)
E2E_PARAMS = dict(min_run=1, max_gap=1000, max_shift=300)  # (deletions of up to 300 bases are links)
E2E_MIN_FRAC = 0.5
READ_LEN, READ_STEP = 100, 10
HARD_AT = {"near_snps": (2, 8000), "tandem": (2, 8400)}  # (contig, first base): excluded from the truth check, not from the model's
HARD_SPAN = 60
TANDEM = b"ACGACGACGACG"  # four units of three bases: shorter than k


def planted():
    """(A, B, edits): A's three contigs, B = A with the edits (contig, pos, ref length, alt) carried out — SNPs, 3-base MNPs,
    insertions of 1 to 90 bases and deletions of 1 to 300 bases, 100 to 400 bases apart and 300 from the contigs' ends — and the
    two hard sites: two SNPs five bases apart, and one more unit of a tandem repeat"""
    rng = np.random.default_rng(2024)
    a, edits = [], []
    for c, L in enumerate(E2E_LENS):
        x = bytearray(sr.ascii_of(sr.random_codes(L, 300 + c)))
        end = L - 300 if c != 2 else HARD_AT["near_snps"][1] - 300
        mine, q, kind = [], 300, c
        while True:
            q += int(rng.integers(100, 401))
            kind += 1
            what = kind % 4
            n = int(rng.integers(1, 301)) if what == 3 else 0
            if q + n + 100 > end:
                break
            if what == 0:
                mine.append(vr._edit_snp(x, q))
            elif what == 1:
                mine.append((q, 3, bytes(vr._other(x[q + i]) for i in range(3))))
            elif what == 2:
                mine.append(vr._edit_ins(x, q, int(rng.integers(1, 91)), 1000 + q))
            else:
                vr._fix_del(x, q, n)
                mine.append((q, n, b""))
            q += n
        if c == 2:
            h = HARD_AT["near_snps"][1]
            mine += [vr._edit_snp(x, h), vr._edit_snp(x, h + 5)]
            t = HARD_AT["tandem"][1]
            x[t - 1:t + len(TANDEM) + 1] = b"T" + TANDEM + b"T"
            mine.append((t, 0, TANDEM[:3]))
        a.append(bytes(x))
        edits.append(sorted(mine))
    b = [vr.plant(x, es) for x, es in zip(a, edits)]
    return a, b, edits


def is_hard(contig, pos):
    return any(c == contig and h - HARD_SPAN <= pos < h + HARD_SPAN for c, h in HARD_AT.values())


def read_starts(L):
    """error-free reads of READ_LEN bases every READ_STEP bases, and one that ends with the contig"""
    s = list(range(0, L - READ_LEN + 1, READ_STEP))
    return s + ([L - READ_LEN] if (L - READ_LEN) % READ_STEP else [])


def reads_of(contigs):
    return [c[s:s + READ_LEN] for c in contigs for s in read_starts(len(c))]


def read_weights(contigs, k):
    """per contig, how many reads of ``reads_of`` hold the window at every k-mer position"""
    out = []
    for c in contigs:
        w = np.zeros(max(len(c) - k + 1, 0), np.int64)
        for s in read_starts(len(c)):
            w[s:s + READ_LEN - k + 1] += 1
        out.append(w)
    return out


def fastq_text(reads, tag="r"):
    return b"".join(b"@%s%d\n%s\n+\n%s\n" % (tag.encode(), i, r, b"I" * len(r)) for i, r in enumerate(reads))


def samples():
    """name -> (the genomes whose contigs the sample is made of — a list of lists of contigs —, truth(contig) -> GT)"""
    a, b, _ = planted()
    return {"reads_a": ([a], lambda c: "0/0"), "reads_b": ([b], lambda c: "1/1"), "reads_ab": ([a, b], lambda c: "0/1"),
            "mosaic": ([[a[0], b[1], b[2]]], lambda c: "0/0" if c == 0 else "1/1")}


class _Unpack:
    def __init__(self, contigs):
        self.contigs = [vr.norm(c) for c in contigs]

    def unpack(self, c):
        return self.contigs[c]


def e2e_sites(k):
    """(sites as table_rows takes them, anchor bases, ranges of A, ranges of B, the variants' frame) of the planted genomes by the numpy models of the
    runs and of the variants (tests/synteny_ref.py, tests/variants_ref.py) under panagram_amd.synteny.variant_frame"""
    from panagram_amd import synteny
    a, b, _ = planted()
    m = vr.variants(sr.segments(a, b, k)[0], a, b, k, **E2E_PARAMS)
    rec = m["records"]
    frame = synteny.variant_frame(*(rec[:, i] for i in range(7)), m["words"][:, 0], m["words"][:, 1], E2E_CHROMS, [len(c) for c in b],
                                  E2E_CHROMS, _Unpack(a), _Unpack(b))
    sites = [(r.chrA, int(r.posA), int(r.refLen), r.chrB, int(r.posB), int(r.altLen), r.strand, r[7], r.ref, r.alt)
             for r in frame.itertuples(index=False)]
    ra = [(E2E_CHROMS.index(s[0]), s[1], s[2]) for s in sites]
    rb = [(E2E_CHROMS.index(s[3]), s[4], s[5]) for s in sites]
    return sites, list(frame.attrs["anchor"]), ra, rb, frame


_E2E_CACHE = {}


def e2e_model(k, sample, fasta=False, min_count=None, min_frac=E2E_MIN_FRAC):
    """dict of the model's ``rows`` (table_rows), ``anchors``, ``reads``, ``hits``, ``support`` (ref, alt), ``min_count``, ``frame``
    (the variants) for one of ``samples()``: as reads (FASTQ, min_count 2) or, ``fasta``, as an assembly (min_count 1)"""
    key = (k, sample, fasta, min_count, min_frac)
    if key in _E2E_CACHE:
        return _E2E_CACHE[key]
    if ("sites", k) not in _E2E_CACHE:
        a, b, _ = planted()
        sites, anchors, ra, rb, frame = e2e_sites(k)
        t = Table(k, 3)
        t.insert_ranges(a, ra)
        t.insert_ranges(b, rb)
        t.count(0, counts_of(a, k))
        t.count(1, counts_of(b, k))
        _E2E_CACHE[("sites", k)] = (a, b, sites, anchors, ra, rb, frame, t)
    a, b, sites, anchors, ra, rb, frame, base = _E2E_CACHE[("sites", k)]
    t = Table(k, 3)
    t.keys, t.planes = base.keys, [base.planes[0], base.planes[1], {}]
    min_count = (1 if fasta else 2) if min_count is None else min_count
    reads = hits = 0
    for genome in samples()[sample][0]:
        if fasta:
            hits += t.count(2, counts_of(genome, k))
            reads += len(genome)
        else:
            hits += t.count(2, counts_of(genome, k, read_weights(genome, k)))
            reads += sum(len(read_starts(len(c))) for c in genome)
    sup = (t.support(a, ra, 0, 1, 2, min_count), t.support(b, rb, 1, 0, 2, min_count))
    out = dict(rows=table_rows(sites, sup[0], sup[1], min_frac), anchors=anchors, reads=reads, hits=hits, support=sup, min_count=min_count,
               frame=frame, min_frac=min_frac)
    _E2E_CACHE[key] = out
    return out


def truth_rows(model, sample):
    """(row, the planted GT) of every site of the model's table but the hard ones"""
    truth = samples()[sample][1]
    return [(r, truth(E2E_CHROMS.index(r[0]))) for r in model["rows"] if not is_hard(E2E_CHROMS.index(r[0]), r[1])]
