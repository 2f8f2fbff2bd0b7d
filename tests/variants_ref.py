"""The variants pg_variants.hip reads off the links of the synteny blocks, restated in numpy by a plain loop; the model's own
``apply``; the planted differences; and the crafted run list that holds every edge k_link_variants has.  No tests in here:
tests/test_variants_cpu.py ties the restatement to cases whose variants follow by construction, tests/test_gpu_run_variants.py
and tests/test_gpu_synteny_variants.py hold the kernel to it.

Definitions (the header of panagram_amd/csrc/pg_variants.hip in the same words); run, kept, predecessor, link, dA, dB and strand
σ are those of tests/blocks_ref.py.  For a link i -> j write p = e_i - 1, the A position of run i's last k-mer; s = s_j; bl = the
B position of run i's last k-mer; b = b_j.  Positions of A are contig-relative, positions of B global, as in the mate words.
  overlap     t = max(0, k - min(dA, dB)); min(dA, dB) >= 1, so t <= k - 1.  The two matched flanks overlap by t bases on the
              shorter side, and the difference is placed at the leftmost place in A that the flanks allow.
  A allele    bases [posA, posA + lenA) of the contig of A, posA = p + k - t, lenA = dA - k + t.  Base posA - 1 is the anchor base.
  B allele    lenB = dB - k + t bases: [bl + k - t, b) on strand 0, [b + k, bl + t) on strand 1; posB is the lowest base of that
              range.  "In A's orientation": as stored on strand 0, reverse-complemented on strand 1.
  mismatches  only when lenA == lenB: the i in [0, lenA) where the facing bases differ or either is non-ACGT.  0 otherwise.
  class       0 same: lenA == lenB and mismatches == 0 — counted, never emitted; 1 snp: lenA == lenB == 1, mismatches == 1; 2 mnp:
              lenA == lenB >= 2, mismatches >= 1; 3 ins: lenA == 0 < lenB; 4 del: lenB == 0 < lenA; 5 complex: both positive and
              unequal.
  N flag      either allele range holds a non-ACGT base.
  record      one per link of class != 0: contig of A, posA, lenA, posB, lenB, info = σ | class << 1 | code of A base posA - 1 << 4
              | N flag << 6, mismatches, and two 64-bit words: the first min(len, 32) bases of either allele in A's orientation,
              base i at bits 2i and 2i + 1 (a non-ACGT base is stored as code 0, so it reads 3 once complemented).
  Records are sorted by (contig of A, run j).
  Invariant: for every block, A's bases from the first run's start to the last run's end + k - 1 with each record's A allele
  replaced by its B allele in A's orientation are B's range of the block, reverse-complemented on strand 1."""
import numpy as np

from tests import blocks_ref as br
from tests import synteny_ref as sr

CLASSES = ("same", "snp", "mnp", "ins", "del", "complex")
SAME, SNP, MNP, INS, DEL, COMPLEX = range(6)
FIELDS = ("contig", "posA", "lenA", "posB", "lenB", "info", "mismatches")
MAX_GAP = 65536
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
_CODE = {65: 0, 67: 1, 71: 2, 84: 3}


def norm(seq: bytes) -> bytes:
    """upper case, N for every byte outside ACGT: what SeqSet.unpack shows"""
    return bytes(c if c in _CODE else 78 for c in bytes(seq).upper())


def revcomp(seq: bytes) -> bytes:
    return bytes(seq).translate(_COMP)[::-1]


def word(allele: bytes, complemented: bool) -> int:
    """the first 32 bases as the kernel packs them: a non-ACGT base is code 0 in the planes, 3 behind a complement"""
    w = 0
    for i, c in enumerate(allele[:32]):
        w |= _CODE.get(c, 3 if complemented else 0) << (2 * i)
    return w


def variants(runs, contigs_a, contigs_b, k, min_run, max_gap, max_shift):
    """the links of the blocks of ``runs`` ([n, 4] = contig, start, end, mate word) over two sides of ASCII contigs: a dict of
    ``records`` [n, 7] int64 = FIELDS, ``words`` [n, 2] uint64, ``alleles`` [(ref, alt)] whole and in A's orientation, ``classes``
    [6] the links of every class, ``links``, and ``blocks``: per block (contig, start of the first run, end of the last, first
    mate word, last mate word of the last run, [indices of its records])"""
    a, b = [norm(c) for c in contigs_a], [norm(c) for c in contigs_b]
    lens_b = [len(c) for c in b]
    offs = np.concatenate([[0], np.cumsum(lens_b)]).astype(np.int64)
    recs, words, alleles, blocks = [], [], [], []
    classes = [0] * 6
    prev = None  # the last kept run
    for run in (tuple(int(x) for x in r) for r in np.asarray(runs, np.int64).reshape(-1, 4)):
        c, s, e, m = run
        n = e - s
        if n < min_run:
            continue
        linked = prev is not None and prev[0] == c and br.link(prev, run, lens_b, max_gap, max_shift)[0]
        if not linked:
            blocks.append([c, s, e, m, br.last_mate(m, n), []])
        else:
            blk = blocks[-1]
            blk[2], blk[4] = e, br.last_mate(m, n)
            p = prev[2] - 1
            bl, bj, strand = br.last_mate(prev[3], prev[2] - prev[1]) >> 1, m >> 1, m & 1
            d_a, d_b = s - p, (bl - bj if strand else bj - bl)
            t = max(0, k - min(d_a, d_b))
            pos_a, len_a, len_b = p + k - t, d_a - k + t, d_b - k + t
            pos_b = bj + k if strand else bl + k - t
            cb = br.contig_of(bl, lens_b)
            lo = pos_b - int(offs[cb])
            assert len_a >= 0 and len_b >= 0 and pos_a >= 1 and pos_a + len_a <= len(a[c]) and 0 <= lo and lo + len_b <= len(b[cb])
            ref, alt = a[c][pos_a:pos_a + len_a], b[cb][lo:lo + len_b]
            alt = revcomp(alt) if strand else alt
            mism = sum(1 for x, y in zip(ref, alt) if x != y or x == 78 or y == 78) if len_a == len_b else 0
            if len_a == len_b:
                cls = SAME if mism == 0 else (SNP if len_a == 1 else MNP)
            else:
                cls = INS if len_a == 0 else (DEL if len_b == 0 else COMPLEX)
            classes[cls] += 1
            if cls != SAME:
                anchor = a[c][pos_a - 1]
                info = strand | cls << 1 | _CODE.get(anchor, 0) << 4 | int(78 in ref or 78 in alt) << 6
                blk[5].append(len(recs))
                recs.append([c, pos_a, len_a, pos_b, len_b, info, mism])
                words.append([word(ref, False), word(alt, bool(strand))])
                alleles.append((ref, alt))
        prev = run
    return dict(records=np.array(recs, np.int64).reshape(-1, 7), words=np.array(words, np.uint64).reshape(-1, 2), alleles=alleles,
                classes=classes, links=sum(classes), blocks=blocks)


def apply(contig_a: bytes, start: int, end: int, edits):
    """bases [start, end) of ``contig_a`` with every edit (posA, lenA, alt) — sorted, apart — carried out"""
    out, at = [], start
    for pos, n, alt in edits:
        assert at <= pos and pos + n <= end
        out += [contig_a[at:pos], alt]
        at = pos + n
    return b"".join(out + [contig_a[at:end]])


def block_b_range(blk, contigs_b, k):
    """B's bases of a block in A's orientation"""
    _, _, _, mf, ml, _ = blk
    lens_b = [len(c) for c in contigs_b]
    strand = mf & 1
    lo, hi = ((mf >> 1), (ml >> 1) + k) if strand == 0 else ((ml >> 1), (mf >> 1) + k)
    cb = br.contig_of(lo, lens_b)
    off = sum(lens_b[:cb])
    seq = norm(contigs_b[cb])[lo - off:hi - off]
    return revcomp(seq) if strand else seq


def invariant_holds(model, contigs_a, contigs_b, k):
    """every block of ``variants``' result: A with the block's records applied is B's range of the block"""
    for blk in model["blocks"]:
        c, s, e = blk[:3]
        edits = [(int(model["records"][i][1]), int(model["records"][i][2]), model["alleles"][i][1]) for i in blk[5]]
        if apply(norm(contigs_a[c]), s, e + k - 1, edits) != block_b_range(blk, contigs_b, k):
            return False
    return True


# ---------------------------------------------------------------------------
# planted differences
# ---------------------------------------------------------------------------
def plant(seq: bytes, edits):
    """``seq`` with every edit (pos, ref length, alt bytes) carried out: B's side of a contig of A"""
    return apply(bytes(seq), 0, len(seq), sorted(edits))


def _other(c, *avoid):
    """a base that differs from ``c`` and from every base of ``avoid``"""
    return next(x for x in b"ACGT" if x != c and x not in avoid)


def _rand(n, seed):
    return sr.ascii_of(sr.random_codes(n, seed))


def _edit_snp(x, q):
    return (q, 1, bytes([_other(x[q])]))


def _edit_ins(x, q, n, seed):
    """n bases in front of base q whose ends do not let either flank run on"""
    ins = bytearray(_rand(n, seed))
    ins[0] = _other(x[q])
    ins[-1] = _other(x[q - 1], x[q] if n == 1 else 0)
    return (q, 0, bytes(ins))


def _fix_del(x, q, n):
    """bases around a deletion [q, q + n) set so that neither flank runs on across it"""
    x[q - 1], x[q], x[q + n - 1], x[q + n] = b"GATC"


def _expect(contig, edits, strand=0):
    """what the model must return for planted edits: (contig, posA, class, ref, alt, strand)"""
    out = []
    for pos, n, alt in sorted(edits):
        cls = (SNP if n == 1 else MNP) if n == len(alt) else (INS if n == 0 else (DEL if not alt else COMPLEX))
        out.append((contig, pos, cls, n, alt, strand))
    return out


def planted_cases(k):
    """name -> (contigs of A, contigs of B, parameters, expected records): ASCII contigs; expected = (contig of A, posA, class,
    ref as a length in A or as bytes, alt in A's orientation, strand) per record in order — None where the case only feeds the
    invariant.  Callers assert that all k-mers of A are distinct where the case says so."""
    wide = dict(min_run=1, max_gap=1000, max_shift=100)
    cases = {}
    codes = br.planted_cases(k)
    asc = lambda side: [sr.ascii_of(c) for c in side]
    # the blocks' own cases
    a, b = asc(codes["snps"][0]), asc(codes["snps"][1])
    cases["snps"] = (a, b, wide, [(ci, q, SNP, 1, b[ci][q:q + 1], 0) for ci in (0, 1) for q in br.SNPS[ci]])
    a, b = asc(codes["indel"][0]), asc(codes["indel"][1])
    cases["indel"] = (a, b, wide, [(0, br.INS_AT, INS, 0, b[0][br.INS_AT:br.INS_AT + br.INS_LEN], 0), (0, br.DEL_AT, DEL, br.DEL_LEN, b"", 0)])
    a, b = asc(codes["stray"][0]), asc(codes["stray"][1])
    n = k + br.STRAY_KMERS - 1
    cases["stray"] = (a, b, dict(min_run=br.STRAY_KMERS + 1, max_gap=1000, max_shift=100), [(0, 400, MNP, n, b[0][400:400 + n], 0)])
    for name in ("inversion", "translocation", "three_b"):
        cases[name] = (asc(codes[name][0]), asc(codes[name][1]), wide, None)

    # an inversion of 300 bases that holds a SNP, an insertion and a deletion: strand 1
    x = bytearray(_rand(900, 101))
    _fix_del(x, 520, 6)
    edits = [_edit_snp(x, 360), _edit_ins(x, 430, 5, 102), (520, 6, b"")]
    inner = plant(bytes(x[300:600]), [(q - 300, n, alt) for q, n, alt in edits])
    cases["inverted"] = ([bytes(x)], [bytes(x[:300]) + revcomp(inner) + bytes(x[600:])], wide, _expect(0, edits, 1))

    # a deletion and an insertion of one unit inside a tandem repeat shorter than k: the flanks overlap, t = 2 r
    r = 4
    assert 2 * r < k
    unit = b"ACGG"
    left, mid, right = bytearray(_rand(300, 104)), bytearray(_rand(300, 105)), bytearray(_rand(300, 106))
    left[-1], mid[0], mid[-1], right[0] = _other(unit[-1]), _other(unit[0]), _other(unit[-1]), _other(unit[0])
    a0 = bytes(left) + unit * 3 + bytes(mid) + unit * 2 + bytes(right)
    b0 = bytes(left) + unit * 2 + bytes(mid) + unit * 3 + bytes(right)
    q_ins = 300 + 3 * r + 300
    cases["tandem"] = ([a0], [b0], wide, [(0, 300, DEL, r, b"", 0), (0, q_ins, INS, 0, unit, 0)])

    # two SNPs fewer than k apart: one mnp; a SNP beside an insertion: complex
    x = bytearray(_rand(900, 107))
    ins = bytearray(_rand(4, 108))
    ins[-1] = _other(x[500], x[501])
    near = (200, 6, bytes([_other(x[200])]) + bytes(x[201:205]) + bytes([_other(x[205])]))
    cplx = (500, 1, bytes([_other(x[500])]) + bytes(ins))
    edits = [near, cplx]
    cases["near"] = ([bytes(x)], [plant(bytes(x), edits)], wide, _expect(0, edits))

    # alleles beyond 32 bases: a 40-base insertion and a 70-base mnp
    x = bytearray(_rand(1200, 109))
    sub = bytearray(_rand(70, 110))
    for i in range(70):  # (every base differs: no k-mer of the stretch survives, and the ends stop the flanks)
        sub[i] = _other(x[700 + i]) if sub[i] == x[700 + i] else sub[i]
    edits = [_edit_ins(x, 300, 40, 111), (700, 70, bytes(sub))]
    cases["long"] = ([bytes(x)], [plant(bytes(x), edits)], wide, _expect(0, edits))

    # an N inside an allele, on either side, and an N-free `same` link made by a k-mer that A and B hold twice
    x = bytearray(_rand(1000, 112))
    x[600] = ord("N")                                     # an N of A facing a base of B
    y = bytearray(x)
    y[600] = ord("C")
    y[300] = ord("N")                                     # a base of A facing an N of B
    y[798], y[800] = _other(x[798]), ord("N")             # three bases, the last one N in B
    dup = bytes(x[100:100 + k])
    before, behind = bytearray(_rand(100, 113)), bytearray(_rand(100, 114))
    before[-1], behind[0] = _other(x[99]), _other(x[100 + k])  # (the one k-mer, not the one beside it too)
    extra = bytes(before) + dup + bytes(behind)
    cases["n_and_dup"] = ([bytes(x), extra], [bytes(y), extra], wide,
                          [(0, 300, SNP, 1, b"N", 0), (0, 600, SNP, 1, b"C", 0), (0, 798, MNP, 3, bytes(y[798:801]), 0)])

    # strand-1 variants whose B alleles lie near the start of B's first contig, the last one within its first 32 bases: B's
    # first contig is A's, reverse-complemented whole, so A's last bases are B's first
    x = bytearray(_rand(400, 115))
    _fix_del(x, 335, 3)
    edits = [(335, 3, b""), _edit_ins(x, 362, 6, 120), (382, 2, bytes([_other(x[382]), _other(x[383])]))]
    tail = _rand(300, 116)
    cases["b_start"] = ([bytes(x), tail], [revcomp(plant(bytes(x), edits)), tail], wide, _expect(0, edits, 1))

    # a strand-0 variant within 32 bases of a contig's end (the last contig of both sides)
    head = _rand(300, 117)
    x = bytearray(_rand(333, 118))
    edits = [_edit_snp(x, 333 - k - 3), _edit_ins(x, 280, 3, 119)]
    cases["a_end"] = ([head, bytes(x)], [head, plant(bytes(x), edits)], wide, _expect(1, edits))
    return cases


def case_runs(case, k):
    """(runs, mated positions of A) of a planted case, by the numpy model of the runs"""
    return sr.segments(case[0], case[1], k)


# ---------------------------------------------------------------------------
# the crafted run list: no hashing, the kernel compares whatever bases lie at the coordinates
# ---------------------------------------------------------------------------
CRAFTED_K = 15
CRAFTED_PARAMS = dict(min_run=3, max_gap=5000, max_shift=60)
CHUNK, TILE, WAVE = br.CHUNK, br.TILE, br.WAVE


class _Lay:
    """the runs of one contig of A laid one behind the other, as tests/blocks_ref.py lays them: a kept run by its link operands
    (dA, dB) against the last kept run, a dropped run right behind the last run of any kind with its mate in B's last contig.
    B positions are relative until ``place`` moves them."""

    def __init__(self, stray):
        self.runs = []      # [s, e, b, strand, kept]
        self.kept = None    # (e, bl, strand) of the last kept run
        self.stray = stray  # [next relative position in B's last contig]

    def first(self, s, b, strand, n=4):
        assert not self.runs or s >= self.runs[-1][1]
        self.runs.append([s, s + n, b, strand, True])
        self.kept = (s + n, b - (n - 1) if strand else b + (n - 1), strand)
        return len(self.runs) - 1

    def add(self, d_a, d_b, n=4, strand=None):
        e, bl, st = self.kept
        strand = st if strand is None else strand
        return self.first(e - 1 + d_a, bl - d_b if strand else bl + d_b, strand, n)

    def drop(self, n=1, gap=1):
        assert n < CRAFTED_PARAMS["min_run"]
        self.stray[0] += 3
        self.runs.append([self.runs[-1][1] + gap if self.runs else 0, 0, self.stray[0], 0, False])
        self.runs[-1][1] = self.runs[-1][0] + n
        return len(self.runs) - 1

    def extent_a(self, k):
        return self.runs[-1][1] + k - 1 if self.runs else 0

    def kept_b(self):
        """(lowest, highest + 1) base of B that a kept run's k-mers touch, relative"""
        lo = min((b - (e - s - 1) if st else b) for s, e, b, st, kp in self.runs if kp)
        hi = max((b if st else b + (e - s - 1)) for s, e, b, st, kp in self.runs if kp)
        return lo, hi + CRAFTED_K


# the link operands the long contigs cycle through, k = 15: substitutions of 1, 3, 20, 40 and 70 bases; flanks that overlap
# without a difference (7, 7); an insertion and a deletion of 2, of 4 inside overlapping flanks (t = 10), of 33; and complex pairs —
# every shifted link is followed by its mirror image, so the runs come back to the diagonal they left
def _cycle(k):
    return [(k + 1, k + 1), (k + 1, k + 1), (k + 3, k + 3), (7, 7), (k, k + 2), (k + 1, k + 1), (k + 2, k), (k + 1, k + 1), (5, 9),
            (k + 2, k + 2), (9, 5), (k + 20, k + 20), (k + 2, k + 5), (k + 1, k + 1), (k + 5, k + 2), (k + 40, k + 40), (k, k + 33),
            (k + 1, k + 1), (k + 33, k), (k + 70, k + 70), (k + 1, k + 1), (k + 31, k + 31), (k + 1, k + 1), (k + 1, k + 1)]


def crafted():
    """(runs [n, 4] int64, contigs of A, contigs of B, k, parameters, marks): ``marks`` names the run indices (inside the whole
    list) that the tests look for: the links across a wave's, a tile's and two chunks' edges, and the pairs at the bounds."""
    k = CRAFTED_K
    G, S = CRAFTED_PARAMS["max_gap"], CRAFTED_PARAMS["max_shift"]
    cyc = _cycle(k)
    stray = [10]
    marks = {}

    # contig 0, strand 0: 3 chunks and 77 runs.  Dropped runs as the first and last lane of a tile and on both sides of a chunk
    # edge, a break in front of run 300 and a strand flip in front of run 8501
    c0 = _Lay(stray)
    c0.first(5, 0, 0)
    dropped = (512, 767, 2 * CHUNK - 1, 2 * CHUNK)
    for i in range(1, 3 * CHUNK + 77):
        if i in dropped:
            c0.drop()
        elif i == 300:
            c0.add(k + 1, G + 100)     # (past max_gap on B: a break; the B positions go on 5000 further)
        elif i == 8501:
            c0.add(k + 1, k + 1, strand=1)
        elif i > 8501:
            c0.add(*cyc[i % len(cyc)][::-1])
        else:
            c0.add(*cyc[i % len(cyc)])

    # contig 1, strand 1 throughout: 4098 runs, its last runs reach the last bases of A's contig = the first of B's first contig,
    # and its last link is an insertion whose five bases of B end below base 32
    c1 = _Lay(stray)
    c1.first(3, 0, 1)
    for i in range(1, CHUNK + 1):
        c1.add(*cyc[i % len(cyc)])
    c1.add(k, k + 5)

    # contig 2: a chunk of kept runs, a chunk whose runs are ALL dropped, and a run that links across it, two chunks back
    c2 = _Lay(stray)
    c2.first(0, 0, 0)
    for i in range(1, CHUNK):
        c2.add(*cyc[i % len(cyc)])
    for i in range(CHUNK):
        c2.drop(gap=0)
    c2.add(CHUNK + k + 3, CHUNK + k + 3)
    for i in range(9):
        c2.add(k + 1, k + 1)

    # contig 3: every bound of max_gap and max_shift and one past each, on strand 0 and, mirrored, on strand 1
    steps = [(G, G - S), (G + 1, G + 1 - S), (G - S, G), (G + 1 - S, G + 1), (20, 20 + S), (20, 21 + S), (20 + S, 20), (21 + S, 20), (k + 1, k + 1)]
    c3 = _Lay(stray)
    c3.first(0, 0, 0)
    for d_a, d_b in steps:
        c3.add(d_a, d_b)
    c4 = _Lay(stray)
    c4.first(0, 0, 1)
    for d_a, d_b in steps:
        c4.add(d_a, d_b)

    # contigs 5 - 7: no run, one kept run, one dropped run
    c5, c6, c7 = _Lay(stray), _Lay(stray), _Lay(stray)
    c6.first(3, 0, 0, n=3)
    c7.drop(2)

    lays = [c0, c1, c2, c3, c4, c5, c6, c7]
    # A's contigs: random, as long as their runs reach; contig 1 ends right behind its last k-mer
    len_a = [max(lay.extent_a(k) + (0 if i == 1 else 37), 50) for i, lay in enumerate(lays)]
    contigs_a = [bytearray(_rand(n, 200 + i)) for i, n in enumerate(len_a)]
    # B: per laid contig of A one contig of B that holds its kept runs, copied from A along the runs' first diagonal with a
    # twentieth of the bases changed (strand 1: reverse-complemented), then the contig of the dropped runs' mates
    rng = np.random.default_rng(300)
    contigs_b, base = [], []
    order = [1, 0, 2, 3, 4, 6]  # (contig 1's B comes first: its strand-1 alleles lie at the start of B's first contig)
    off = 0
    for ci in order:
        lay = lays[ci]
        lo, hi = lay.kept_b()
        pad = 0 if ci == 1 else 41
        n = hi - lo + 2 * pad
        seq = bytearray(_rand(n, 400 + ci))
        # the diagonal of the first kept run: A position s faces relative B position b (strand 0) / b + k - 1 (strand 1)
        s0, _, b0, st, _ = next(r for r in lay.runs if r[4])
        src = bytes(contigs_a[ci])
        for q in range(n):
            rel = q - pad + lo                                     # the relative B position of base q
            pa = s0 + (rel - b0) if st == 0 else s0 + (b0 + k - 1 - rel)
            if 0 <= pa < len(src) and rng.random() >= 0.05:
                seq[q] = src[pa] if st == 0 else src[pa:pa + 1].translate(_COMP)[0]
        contigs_b.append(seq)
        base.append((ci, off + pad - lo))                          # relative -> global
        off += n
    nstray = stray[0] + 3 + k + 2
    contigs_b.append(bytearray(_rand(nstray, 500)))
    stray_base = off
    # non-ACGT bases: a few on either side, inside the stretches the long contigs' alleles cover
    for ci in (0, 1, 2):
        for q in range(1000 + 7 * ci, len(contigs_a[ci]) - 100, 5003):
            contigs_a[ci][q] = ord("N")
    for seq in contigs_b[:3]:
        for q in range(1500, len(seq) - 100, 7001):
            seq[q] = ord("n")
    shift = dict(base)
    rows = []
    first_row = []
    for ci, lay in enumerate(lays):
        first_row.append(len(rows))
        for s, e, b, st, kp in lay.runs:
            rows.append((ci, s, e, ((b + (shift[ci] if kp else stray_base)) << 1) | st))
    marks["wave"] = first_row[0] + WAVE          # the run whose predecessor is the last lane of the wave before
    marks["tile"] = first_row[0] + TILE          # ... of the tile before
    marks["chunk"] = first_row[0] + CHUNK        # ... of the chunk before
    marks["two_chunks"] = first_row[2] + 2 * CHUNK  # ... of a chunk two chunks back, only dropped runs between
    marks["bounds"] = (first_row[3], first_row[4])  # run r + 1 + i of either contig is pair i of `steps`
    marks["steps"] = steps
    marks["first_row"] = first_row
    return (np.array(rows, np.int64), [bytes(c) for c in contigs_a], [bytes(c) for c in contigs_b], k, dict(CRAFTED_PARAMS), marks)
