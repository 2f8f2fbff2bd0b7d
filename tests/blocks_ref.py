"""The blocks pg_blocks.hip chains from the runs of unique matches, restated in numpy by a plain loop, and the crafted run list
that holds every edge k_run_blocks has.  No tests in here: tests/test_blocks_cpu.py ties the restatement to cases whose blocks
follow by construction, tests/test_gpu_run_blocks.py and tests/test_gpu_synteny_blocks.py hold the kernel to it.

Definitions (the header of panagram_amd/csrc/pg_blocks.hip in the same words):
  run          what pg_mate_runs emits (tests/synteny_ref.py: runs): the contig c of A, k-mer positions [s, e) of that contig,
               n = e - s, the mate word m of position s, the strand σ = m & 1, b = m >> 1.  The B position of the run's last k-mer
               is bl = b + (n - 1) on strand 0 and bl = b - (n - 1) on strand 1; its mate word is ml = bl << 1 | σ.  Runs are
               sorted by (c, s).
  kept         a run with n >= min_run.  Dropped runs do not exist for anything below.
  predecessor  of a kept run j: the nearest kept run i before it in the same contig of A, any number of dropped runs between.
  link i -> j  dA = s_j - (e_i - 1), always >= 1; dB = b_j - bl_i on strand 0, bl_i - b_j on strand 1; signed.  The link exists
               iff  σ_i == σ_j,  1 <= dA <= max_gap,  1 <= dB <= max_gap,  |dA - dB| <= max_shift,  and the global B positions
               bl_i and b_j lie in the same contig of B.
  same/shifted a link is same when dA == dB, shifted otherwise.
  block        a maximal chain of kept runs, each linked to its predecessor: (contig of A, start = s of the first run, end = e of
               the last, mate_first = m of the first, mate_last = ml of the last, kmers = the sum of n, runs, shifted links),
               sorted by (contig, start).
With min_run = 1 and max_gap = 1 the blocks are exactly the runs."""
import numpy as np

from tests import synteny_ref as sr

CHUNK, TILE, WAVE = 4096, 256, 64
COLUMNS = ("contig", "start", "end", "mate_first", "mate_last", "kmers", "runs", "shifted")


def contig_of(pos, lens_b):
    """the contig of B that holds global position ``pos`` (an empty contig holds none)"""
    ends = np.cumsum(np.asarray(lens_b, np.int64))
    c = int(np.searchsorted(ends, pos, side="right"))  # the first contig that ends behind pos: it starts at or before it
    if pos < 0 or c >= len(ends):
        raise ValueError(f"position {pos} outside genome B")
    return c


def last_mate(m, n):
    return m - 2 * (n - 1) if m & 1 else m + 2 * (n - 1)


def link(run_i, run_j, lens_b, max_gap, max_shift):
    """(linked, shifted) of two kept runs (c, s, e, m) of one contig of A, i the predecessor of j"""
    _, _, e_i, m_i = run_i
    _, s_j, _, m_j = run_j
    if (m_i & 1) != (m_j & 1):
        return False, False
    bl_i, b_j = last_mate(m_i, e_i - run_i[1]) >> 1, m_j >> 1
    d_a = s_j - (e_i - 1)
    d_b = bl_i - b_j if m_j & 1 else b_j - bl_i
    assert d_a >= 1
    if not (1 <= d_a <= max_gap and 1 <= d_b <= max_gap and abs(d_a - d_b) <= max_shift):
        return False, False
    if contig_of(bl_i, lens_b) != contig_of(b_j, lens_b):
        return False, False
    return True, d_a != d_b


def failed_conditions(run_i, run_j, lens_b, max_gap, max_shift):
    """the link conditions that kept runs i -> j of one contig of A do NOT meet, by name: what ``link`` decides, taken apart so
    that a test can ask which condition alone refuses a pair"""
    _, s_i, e_i, m_i = run_i
    _, s_j, _, m_j = run_j
    bl_i, b_j = last_mate(m_i, e_i - s_i) >> 1, m_j >> 1
    d_a = s_j - (e_i - 1)
    d_b = bl_i - b_j if m_j & 1 else b_j - bl_i
    checks = {"strand": (m_i & 1) == (m_j & 1), "dA <= max_gap": d_a <= max_gap, "dB >= 1": d_b >= 1, "dB <= max_gap": d_b <= max_gap,
              "shift": abs(d_a - d_b) <= max_shift, "contig of B": contig_of(bl_i, lens_b) == contig_of(b_j, lens_b)}
    return sorted(name for name, ok in checks.items() if not ok)


def blocks(runs, lens_b, min_run, max_gap, max_shift):
    """[n, 8] int64 = COLUMNS of the blocks of ``runs`` ([n, 4] = contig, start, end, mate word; sorted by (contig, start))"""
    out = []
    prev = None  # the last kept run
    for run in (tuple(int(x) for x in r) for r in np.asarray(runs, np.int64).reshape(-1, 4)):
        c, s, e, m = run
        n = e - s
        if n < min_run:
            continue
        linked, shifted = (False, False)
        if prev is not None and prev[0] == c:
            linked, shifted = link(prev, run, lens_b, max_gap, max_shift)
        if linked:
            blk = out[-1]
            blk[2], blk[4] = e, last_mate(m, n)
            blk[5] += n
            blk[6] += 1
            blk[7] += int(shifted)
        else:
            out.append([c, s, e, m, last_mate(m, n), n, 1, 0])
        prev = run
    return np.array(out, np.int64).reshape(-1, 8)


def block_rows(blks, k, names_a, lens_b, names_b, min_len=1):
    """the block table, one tuple (chrA, startA, endA, chrB, startB, endB, strand, kmers, runs, shifted) per block of at least
    ``min_len`` k-mers, by a plain loop"""
    out = []
    offs = np.concatenate([[0], np.cumsum(np.asarray(lens_b, np.int64))])
    for c, s, e, mf, ml, km, nr, sh in np.asarray(blks, np.int64).reshape(-1, 8).tolist():
        if km < min_len:
            continue
        strand = mf & 1
        lo, hi = ((mf >> 1), (ml >> 1) + k) if strand == 0 else ((ml >> 1), (mf >> 1) + k)
        cb = contig_of(lo, lens_b)
        out.append((names_a[c], s, e + k - 1, names_b[cb], lo - int(offs[cb]), hi - int(offs[cb]), "+-"[strand], km, nr, sh))
    return out


# ---------------------------------------------------------------------------
# the crafted run list
# ---------------------------------------------------------------------------
CRAFTED_PARAMS = dict(min_run=3, max_gap=5000, max_shift=10)
CRAFTED_LENS_B = [3_000_000, 1_000_000, (1 << 31) - 4_000_000]  # B's positions reach 2^31 - 1: the mate word 0xFFFFFFFE


class _Contig:
    """the runs of one contig of A, laid one behind the other: a kept run by its link operands (dA, dB) against the last kept
    run, a dropped run (fewer than min_run k-mers, a stray mate in B's first contig) right behind the last run of any kind"""
    stray = 10

    def __init__(self):
        self.runs = []       # (s, e, m)
        self.kept = None     # (e, bl, strand) of the last kept run

    def _push(self, s, n, b, strand):
        assert not self.runs or s >= self.runs[-1][1], "the runs of a contig are sorted and do not overlap"
        assert n >= 1 and b >= 0 and (b - (n - 1) >= 0 if strand else b + n - 1 < sum(CRAFTED_LENS_B))
        self.runs.append((s, s + n, (b << 1) | strand))
        return len(self.runs) - 1

    def first(self, s, b, strand, n=4):
        self.kept = (s + n, b - (n - 1) if strand else b + (n - 1), strand)
        return self._push(s, n, b, strand)

    def add(self, d_a=7, d_b=7, n=4, strand=None):
        e, bl, st = self.kept
        strand = st if strand is None else strand
        s, b = e - 1 + d_a, (bl - d_b if strand else bl + d_b)
        return self.first(s, b, strand, n)

    def drop(self, n=1, gap=1):
        assert n < CRAFTED_PARAMS["min_run"]
        _Contig.stray += 13
        return self._push(self.runs[-1][1] + gap if self.runs else 0, n, _Contig.stray, 0)


def crafted_runs():
    """(runs [n, 4] int64, contigs of A, lens_b, parameters, want): every edge of k_run_blocks in one run list.  ``want[c]`` is
    written out by hand: the blocks of contig c as (index of the first run, index of the last run, kept runs, shifted links),
    run indices inside the contig."""
    _Contig.stray = 10
    G, S = CRAFTED_PARAMS["max_gap"], CRAFTED_PARAMS["max_shift"]
    contigs, want = [], {}

    # 0: 3 chunks and 77 runs on strand +.  Links across 63|64 and 255|256; a break in front of run 300; ONE block from run 300 to
    # run 8500 over three chunks, every 100th of its links shifted, with kept runs on both sides of 4095|4096 and dropped runs as
    # the first (512) and last (767) of a tile, the last of a chunk (8191) and the first of the next (8192); a strand flip in
    # front of run 8501; the last block reaches the contig's last run
    c = _Contig()
    c.first(5, 5_000_000, 0)
    dropped = (512, 767, 2 * CHUNK - 1, 2 * CHUNK)
    nshift = 0
    for i in range(1, 3 * CHUNK + 77):
        if i in dropped:
            c.drop()
        elif i == 300:
            c.add(7, 6000)
        elif i == 8501:
            c.add(7, 7, strand=1)
        elif i - 1 in dropped:
            c.add(12, 12)
        elif 300 < i <= 8500 and i % 100 == 0:
            c.add(7, 9)
            nshift += 1
        else:
            c.add()
    assert nshift == 82
    want[0] = [(0, 299, 300, 0), (300, 8500, 8201 - 4, 82), (8501, 3 * CHUNK + 76, 3 * CHUNK + 77 - 8501, 0)]
    contigs.append(c)

    # 1: 4097 runs, strand - throughout: no link across 63|64 (dB = 0), 255|256 (dB = -3) and 4095|4096 (a shift of max_shift + 1)
    c = _Contig()
    c.first(0, 2_900_000, 1)
    for i in range(1, CHUNK + 1):
        c.add(*{WAVE: (7, 0), TILE: (7, -3), CHUNK: (7, 7 + S + 1)}.get(i, (7, 7)))
    want[1] = [(0, 63, 64, 0), (64, 255, 192, 0), (256, 4095, 3840, 0), (4096, 4096, 1, 0)]
    contigs.append(c)

    # 2: exactly 4096 runs in B's second contig, the first and the last one dropped
    c = _Contig()
    c.drop(2)
    c.first(10, 3_000_100, 0)
    for i in range(2, CHUNK - 1):
        c.add()
    c.drop(2)
    assert len(c.runs) == CHUNK
    want[2] = [(1, CHUNK - 2, CHUNK - 2, 0)]
    contigs.append(c)

    # 3: a chunk of kept runs, a chunk whose runs are ALL dropped, and a run that links across it (dA = 4098, dB = 4100: shifted)
    c = _Contig()
    c.first(0, 100_000_000, 0)
    for i in range(1, CHUNK):
        c.add()
    for i in range(CHUNK):
        c.drop(gap=0)                  # (one position each, back to back: 4096 positions of A)
    c.add(CHUNK + 2, CHUNK + 4)
    for i in range(9):
        c.add()
    want[3] = [(0, 2 * CHUNK + 9, CHUNK + 10, 1)]
    contigs.append(c)

    # 4 - 7: contigs of 0 runs, 1 kept run, 1 dropped run, 0 runs
    contigs.append(_Contig())
    c = _Contig()
    c.first(3, 777, 0, n=3)
    want[5] = [(0, 0, 1, 0)]
    contigs.append(c)
    c = _Contig()
    c.drop(2)
    contigs.append(c)
    contigs.append(_Contig())

    # 8, 9: two contigs of A whose positions, in A and in B, go on as one block's would: no link across A's contig edge
    c = _Contig()
    c.first(0, 7_000_000, 0)
    c.add()
    c.add()
    want[8] = [(0, 2, 3, 0)]
    contigs.append(c)
    d = _Contig()
    d.kept = c.kept
    d.add()
    d.add()
    want[9] = [(0, 1, 2, 0)]
    contigs.append(d)

    # 10: the contig edge of B at 3 000 000.  A link just below it; a pair five positions apart on either side of it, which
    # satisfies everything else; then the last position of B's first contig and the first of its second, dA = dB = 1
    c = _Contig()
    c.first(0, 2_999_980, 0)           # bl = 2 999 983
    c.add(5, 5, n=4)                   # b = 2 999 988, bl = 2 999 991: linked
    c.add(5, 5, n=4)                   # b = 2 999 996, bl = 2 999 999: linked, ends on the contig's last position
    c.add(1, 1, n=4)                   # b = 3 000 000: the next contig
    c.add(5, 5, n=4)                   # linked, inside the second contig
    c.first(c.kept[0] + 100, 2_999_992, 0, n=4)   # (far away in A) bl = 2 999 995
    c.add(8, 8, n=4)                   # b = 3 000 003: across the edge
    want[10] = [(0, 2, 3, 0), (3, 4, 2, 0), (5, 5, 1, 0), (6, 6, 1, 0)]
    contigs.append(c)

    # 11: every link condition at its bound and one past it, strand +, then a unit step and a strand flip.  A pair past a bound
    # is past that bound ALONE (the other gap inside its bound, the shift at most max_shift), so that each condition decides a
    # pair by itself; a pair at a gap's bound has its shift at max_shift too
    c = _Contig()
    c.first(0, 8_000_000, 0)
    steps = [(G, G - S), (G + 1, G + 1 - S), (G - S, G), (G + 1 - S, G + 1), (20, 20 + S), (20, 21 + S), (20 + S, 20), (21 + S, 20),
             (7, 0), (7, -3), (1, 1)]
    for d_a, d_b in steps:
        c.add(d_a, d_b)
    c.add(7, 7, strand=1)
    #       run: 0 1 | 2 3 | 4 5 | 6 7 | 8 | 9 | 10 11 | 12
    want[11] = [(0, 1, 2, 1), (2, 3, 2, 1), (4, 5, 2, 1), (6, 7, 2, 1), (8, 8, 1, 0), (9, 9, 1, 0), (10, 11, 2, 0), (12, 12, 1, 0)]
    contigs.append(c)

    # 12: the same on strand -, and a flip back to +
    c = _Contig()
    c.first(0, 30_000_000, 1)
    for d_a, d_b in [(G, G - S), (G + 1 - S, G + 1), (20, 20 + S), (20, 21 + S), (7, 0), (7, -3), (G + 1, G + 1 - S)]:
        c.add(d_a, d_b)
    c.add(7, 7, strand=0)
    want[12] = [(0, 1, 2, 1), (2, 3, 2, 1), (4, 4, 1, 0), (5, 5, 1, 0), (6, 6, 1, 0), (7, 7, 1, 0), (8, 8, 1, 0)]
    contigs.append(c)

    # 13: the largest words.  A block on strand + whose last k-mer lies at 2^31 - 1 (mate_last = 0xFFFFFFFE); on strand - a block
    # that starts at the largest odd mate word, 0xFFFFFFFD
    c = _Contig()
    c.first(0, (1 << 31) - 15, 0)      # bl = 2^31 - 12
    c.add(7, 7, n=5)                   # b = 2^31 - 5, bl = 2^31 - 1
    c.first(100, (1 << 31) - 2, 1)     # m = 0xFFFFFFFD
    c.add(7, 9)
    want[13] = [(0, 1, 2, 0), (2, 3, 2, 1)]
    contigs.append(c)

    rows = [(ci, s, e, m) for ci, c in enumerate(contigs) for s, e, m in c.runs]
    return np.array(rows, np.int64), len(contigs), list(CRAFTED_LENS_B), dict(CRAFTED_PARAMS), want


def want_blocks(runs, want):
    """``crafted_runs()``'s hand-written blocks as (contig, start, end, mate_first, mate_last, runs, shifted) rows"""
    runs = np.asarray(runs, np.int64)
    out = []
    for c in sorted(want):
        mine = runs[runs[:, 0] == c]
        for first, last, nruns, shifted in want[c]:
            _, s, _, m = mine[first].tolist()
            _, ls, le, lm = mine[last].tolist()
            out.append([c, s, le, m, last_mate(lm, le - ls), nruns, shifted])
    return np.array(out, np.int64).reshape(-1, 7)


# ---------------------------------------------------------------------------
# planted differences, shared by tests/test_blocks_cpu.py and tests/test_gpu_synteny_blocks.py
# ---------------------------------------------------------------------------
SNPS = ([100, 300, 650], [50, 400])   # in the two planted contigs: more than k apart for k <= 32, and from the contigs' ends
INS_AT, INS_LEN, DEL_AT, DEL_LEN = 300, 7, 600, 5
STRAY_KMERS = 5


def planted_cases(k):
    """name -> (contigs of A, contigs of B) as code arrays: the planted contigs of tests/synteny_ref.py against themselves with
    substitutions, with an insertion and a deletion, with an inversion, with the translocation and the inversion, with a stray
    run, and against a B cut into three contigs.  The bases at every junction are set so that no k-mer spanning it matches by
    chance (callers assert that all k-mers of A are distinct)."""
    x, y = sr.planted_contigs()
    cases = {}
    cases["snps"] = ([x, y], [sr.plant_snps(x, SNPS[0]), sr.plant_snps(y, SNPS[1])])
    # INS_LEN bases put into B in front of base INS_AT, DEL_LEN bases of A from DEL_AT on missing from B
    xi = x.copy()
    xi[[DEL_AT - 1, DEL_AT, DEL_AT + DEL_LEN - 1, DEL_AT + DEL_LEN]] = [2, 0, 3, 1]  # (no match runs on across the deletion)
    ins = sr.random_codes(INS_LEN, 77)
    ins[0], ins[-1] = (xi[INS_AT] + 1) & 3, (xi[INS_AT - 1] + 1) & 3                 # (... nor into the insertion)
    cases["indel"] = ([xi], [np.concatenate([xi[:INS_AT], ins, xi[INS_AT:DEL_AT], xi[DEL_AT + DEL_LEN:]])])
    cases["inversion"] = ([x, y], [x, sr.plant_inversion(y, 100, 140)])
    cases["translocation"] = ([x, y], sr.planted_rearranged(x, y))
    # a stray run: STRAY_KMERS k-mers of A between two collinear stretches lie in ANOTHER contig of B, the stretch between them
    # is B's own
    p, q = x[:400].copy(), x[500:].copy()
    z, r = sr.random_codes(k + STRAY_KMERS - 1, 78), sr.random_codes(k + STRAY_KMERS - 1, 79)
    w1, w2 = sr.random_codes(200, 80), sr.random_codes(150, 81)
    r[0], r[-1] = (z[0] + 1) & 3, (z[-1] + 1) & 3
    w1[-1], w2[0] = (p[-1] + 1) & 3, (q[0] + 1) & 3
    cases["stray"] = ([np.concatenate([p, z, q])], [np.concatenate([p, r, q]), np.concatenate([w1, z, w2])])
    cases["three_b"] = ([x], [x[:300], x[300:600], x[600:]])
    return cases


def case_runs(case, k):
    """(runs, mated positions of A, lens_b) of a planted case"""
    a, b = case
    runs, mated = sr.segments([sr.ascii_of(c) for c in a], [sr.ascii_of(c) for c in b], k)
    return runs, mated, [len(c) for c in b]
