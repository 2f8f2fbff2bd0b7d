"""What pg_novel.hip computes, restated in numpy the obvious way, on tests/screen_ref.py's ``sample_counts`` and tests/copies_ref.py's
``valid_keys``.  The pan table is a set of ``keys`` (distinct canonical k-mers); the sample is a list of sequence sets, each a list
of contigs (ASCII bytes).  No tests in here: tests/test_novel_cpu.py holds the model to a brute-force dict walk and the crafted
sample to its promises, tests/test_gpu_novel*.py hold the kernels to the model.  Oracle side only; never imported by the product.

  valid window   holds no non-ACGT byte; a contig shorter than k has none.  Lower case counts as upper.
  novel key      the canonical key of a valid window of the sample that the table does not hold; depth(key) = the sample's valid
                 windows with that key, over every set, both strands.  solid: depth >= min_count.
  novel run      a maximal [a, b) of consecutive valid positions of ONE contig whose keys are all novel; left_held = position a - 1
                 exists, is valid and the table holds its key; right_held the same of position b.
  bases          max(0, (right_held ? b : b + k - 1) - (left_held ? a + k - 1 : a)): the bases that lie in novel windows only."""
import functools

import numpy as np

from tests import copies_ref as cr
from tests import kmerstats_ref as KR
from tests import screen_ref as SR

BINS = 64
JOB = 1 << 14   # k-mer positions per block of k_novel_count
CHUNK = 4096    # ... per block of k_novel_runs
TILE = 256      # ... per step of a block
WAVE = 64       # ... per wave of a step


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
def novel_counts(keys, sets, k):
    """(windows, hits, novel keys [uint64, sorted], their depths [int64]) of the sample against the table's ``keys``"""
    windows, u, c = SR.sample_counts(sets, k)
    held = np.isin(u, np.asarray(keys, np.uint64))
    return windows, int(c[held].sum()), u[~held], c[~held]


def result(depths, min_count) -> dict:
    """the counts of one pass over the novel table, as engine.NovelTable.result names them"""
    d = np.asarray(depths, np.int64)
    solid = d >= int(min_count)
    return dict(nkeys=int(len(d)), solid=int(solid.sum()), solid_windows=int(d[solid].sum()),
                depth_hist=np.bincount(np.minimum(d, BINS - 1), minlength=BINS).astype(np.int64))


def solid_keys(nkeys, depths, min_count):
    """(keys, depths) of the solid novel k-mers, sorted by key"""
    keep = np.asarray(depths, np.int64) >= int(min_count)
    return np.asarray(nkeys, np.uint64)[keep], np.asarray(depths, np.int64)[keep]


def states(keys, contig, k):
    """per k-mer position of one contig: 0 invalid, 1 held, 2 novel"""
    (key, valid), = cr.keys_of([contig], k)
    return np.where(valid, np.where(np.isin(key, np.asarray(keys, np.uint64)), 1, 2), 0).astype(np.int64)


def runs(keys, contigs, k):
    """(run_contig, run_start, run_end, left_held, right_held [int64 arrays, sorted by (contig, start)], windows, novel_windows)"""
    out = [[], [], [], [], []]
    windows = novel = 0
    for c, seq in enumerate(contigs):
        s = states(keys, seq, k)
        windows += int((s != 0).sum())
        novel += int((s == 2).sum())
        pad = np.concatenate([[0], s, [0]])  # (nothing in front of a contig, nothing behind it)
        is_novel = pad == 2
        a = np.flatnonzero(is_novel[1:-1] & ~is_novel[:-2])      # positions whose predecessor is not novel
        b = np.flatnonzero(is_novel[1:-1] & ~is_novel[2:]) + 1   # exclusive ends
        assert len(a) == len(b)
        for col, v in zip(out, ([c] * len(a), a, b, pad[a] == 1, pad[b + 1] == 1)):
            col.extend(np.asarray(v, np.int64).tolist())
    return (*[np.asarray(col, np.int64) for col in out], windows, novel)


def bases(start, end, left_held, right_held, k):
    a, b = np.asarray(start, np.int64), np.asarray(end, np.int64)
    hi = np.where(np.asarray(right_held, bool), b, b + k - 1)
    lo = np.where(np.asarray(left_held, bool), a + k - 1, a)
    return np.maximum(0, hi - lo)


# ---------------------------------------------------------------------------
# brute force: a dict walk over the windows, one at a time, with its own canonical form
# ---------------------------------------------------------------------------
_DIGITS = bytes.maketrans(b"ACGTacgt", b"01230123")


def brute_key(window: bytes):
    """the canonical key of a window of k bytes, None when it holds a byte outside ACGTacgt"""
    if any(ch not in b"ACGTacgt" for ch in window):
        return None
    return min(int(window.translate(_DIGITS), 4), int(SR.revcomp(window).translate(_DIGITS), 4))


def brute(keys, sets, k):
    """(windows, hits, {novel key: depth}) by a walk over every window of every contig"""
    held = set(int(x) for x in keys)
    windows = hits = 0
    depth = {}
    for contigs in sets:
        for seq in contigs:
            seq = bytes(seq)
            for p in range(len(seq) - k + 1):
                key = brute_key(seq[p:p + k])
                if key is None:
                    continue
                windows += 1
                if key in held:
                    hits += 1
                else:
                    depth[key] = depth.get(key, 0) + 1
    return windows, hits, depth


def brute_runs(keys, contigs, k):
    """[(contig, start, end, left_held, right_held)] by a walk over the positions, one at a time"""
    held = set(int(x) for x in keys)
    out = []
    for c, seq in enumerate(contigs):
        seq = bytes(seq)
        n = len(seq) - k + 1
        st = []
        for p in range(max(n, 0)):
            key = brute_key(seq[p:p + k])
            st.append(0 if key is None else 1 if key in held else 2)
        p = 0
        while p < len(st):
            if st[p] != 2:
                p += 1
                continue
            a = p
            while p < len(st) and st[p] == 2:
                p += 1
            out.append((c, a, p, int(a > 0 and st[a - 1] == 1), int(p < len(st) and st[p] == 1)))
    return out


# ---------------------------------------------------------------------------
# the crafted table and the crafted sample
# ---------------------------------------------------------------------------
HOMOPOLYMER_WINDOWS = 300          # all on one key and one counter: a depth a byte does not hold
SAT3, SAT11 = b"AAC", b"AACCGATGTCT"  # the novel satellites: 3 keys; 11 keys — more slots in a wave than it folds
SAT3_BASES = 200
LONG_POSITIONS = 2 * JOB + 300 + 57  # the period-11 contig: three jobs, the same novel keys on both sides of either job edge
UNIT = 211                         # the period of the backbone the run contigs are cut from: its k-mers are the table's
BACKBONE = CHUNK + 900
INSERTION = 37
EDGES_POSITIONS = 2 * CHUNK + TILE  # the ``edges`` contig: two chunks and one tile, exactly
EXACT_FROM_K = 21                  # from this k on no chance hit splits a planted run or deepens a planted key


def table_size(k):
    """table keys drawn at random: 3000, fewer where the canonical k-mers are few (k = 6 has 2080)"""
    return 3000 if k >= 11 else 300


def _window_keys(seq, k):
    return set(int(x) for x in cr.valid_keys([seq], k))


def _periodic(unit, nbases):
    return (unit * (nbases // len(unit) + 2))[:nbases]


def _rand(rng, n, first_not=None, last_not=None):
    """n random bases; the first is not the byte ``first_not``, the last not ``last_not`` (a planted sequence that began with the
    base behind it, or ended with the base in front of it, would be planted one base further along)"""
    while True:
        s = SR._ACGT[rng.integers(0, 4, n)].tobytes()
        if s[0] != first_not and s[-1] != last_not:
            return s


def _del_at(seq, at, n):
    """the first place from ``at`` on where deleting n bases leaves a junction that no shift of the deletion explains"""
    while seq[at + n] == seq[at] or seq[at + n - 1] == seq[at - 1]:
        at += 1
    return at


@functools.lru_cache(maxsize=None)
def crafted(k, min_count=2, seed=0):
    """(table keys, sets, run contigs, promises) — left alone by every test that shares it.

    The table: ``SR.table_keys`` without the homopolymer's key (the period-3 satellite ACG stays: held), without the keys reserved
    for the novel elements below, and with every k-mer of the backbone, a random unit of UNIT bases repeated.

    The sample, two sequence sets.  Held: keys of the table spelled on either strand, joined by N (and back to back in the second
    set from k = 16 on: the junctions' windows are novel keys of depth 1).  Novel: the homopolymer (HOMOPOLYMER_WINDOWS windows on
    one key), the satellites of period 3 and 11 (the latter LONG_POSITIONS positions in one contig), ``twice`` (once per strand),
    ``edge`` (min_count - 1 times in the first set, once more in the second), ``broken`` (an N in it, then whole), ``lower`` (lower
    case), and contigs of k - 1 and k bases.

    The run contigs, cut from the backbone: ``plain`` (no run), ``start`` / ``end`` (random bases at a contig's start / end),
    ``sub`` (a substitution: bases 1), ``ins`` (INSERTION random bases: bases INSERTION), ``del`` (a deletion: bases 0), ``tile`` /
    ``chunk`` (the homopolymer inserted so that its run crosses position TILE / CHUNK at any k), ``cut`` (an insertion with an N in it: two runs), ``all``
    (a wholly novel contig: bases = its length), ``short`` (k - 1 bases), ``homo`` (ten positions of the homopolymer: held on neither side at any k), ``start_a`` / ``end_a`` (the
    homopolymer at a contig's start / end: a run from the first / to the last position at any k), ``edges`` (substitutions placed so
    that runs start at a wave's, a tile's and a chunk's first position, end with a chunk's last, and reach the end of a contig that
    is a whole number of tiles).  promises["runs"]: name -> contig number."""
    rng = np.random.default_rng(1000 * k + seed)
    drawn = SR.table_keys(rng, table_size(k), k)
    homo = int(drawn[0])
    sat3 = _periodic(SAT3, SAT3_BASES)
    long_c = _periodic(SAT11, LONG_POSITIONS + k - 1)
    reserved = {homo} | _window_keys(sat3, k) | _window_keys(long_c, k)
    assert len(_window_keys(sat3, k)) == 3 and len(_window_keys(long_c, k)) == 11 and len(reserved) == 15
    singles = [int(x) for x in KR.random_keys(rng, 64, k) if int(x) not in reserved][:5]
    twice, edge, broken, lower, exact = singles
    reserved |= set(singles)
    while True:  # (k = 6: a unit may hold a reserved key by chance; the next one)
        backbone = _periodic(_rand(rng, UNIT), BACKBONE)
        bkeys = _window_keys(backbone, k)
        if not bkeys & reserved:
            break
    table = np.array(sorted((set(int(x) for x in drawn[1:]) | bkeys) - reserved), np.uint64)
    plain = np.array([int(x) for x in drawn[1:] if int(x) not in reserved and int(x) not in bkeys], np.uint64)

    def strand(s):
        return s if rng.random() < 0.5 else SR.revcomp(s)

    def spell(key):
        return SR.spell(key, k)
    a, b = [], []
    a += [b"N".join(strand(spell(x)) for x in plain[:200])]
    a += [b"A" * (HOMOPOLYMER_WINDOWS + k - 1) if rng.random() < 0.5 else b"T" * (HOMOPOLYMER_WINDOWS + k - 1)]
    a += [spell(twice)] + [strand(spell(edge)) for _ in range(min_count - 1)]
    s = spell(broken)
    a += [s[:k // 2] + b"N" + s[k // 2 + 1:] + b"n" + strand(s)]
    a += [strand(spell(lower)).lower(), spell(exact)[:k - 1], strand(spell(exact))]
    if k >= 16:
        a += [_rand(rng, 400)]  # (novel keys that only the first set holds: their depths must come through the growth as they are)
    b += [SR.revcomp(spell(twice)), strand(spell(edge)), sat3]
    b += [(b"" if k >= 16 else b"N").join(strand(spell(x)) for x in rng.permutation(plain[:200])[:120])]
    b += [backbone[100:700]]  # (held stretches: no window of theirs may enter the novel table)
    b += [long_c]  # (the second add grows a table that holds keys)

    # the run contigs
    def sub(seq, at):
        return seq[:at] + bytes([b"ACGT"[(b"ACGT".index(seq[at]) + 1 + int(rng.integers(0, 3))) % 4]]) + seq[at + 1:]
    names, R = [], []

    def add(name, seq):
        names.append(name)
        R.append(seq)
    add("plain", backbone[:900])
    add("start", _rand(rng, 50, last_not=backbone[49]) + backbone[50:700])
    add("end", backbone[300:900] + _rand(rng, 45, first_not=backbone[900]))
    add("sub", sub(backbone[:800], 400))
    add("ins", backbone[:500] + _rand(rng, INSERTION, backbone[500], backbone[499]) + backbone[500:1000])
    del_at = _del_at(backbone, 500, 30)
    add("del", backbone[:del_at] + backbone[del_at + 30:1000])
    add("tile", backbone[:TILE - 20] + b"A" * (k + 40) + backbone[TILE - 20:700])
    add("chunk", backbone[:CHUNK - 20] + b"A" * (k + 40) + backbone[CHUNK - 20:])
    add("cut", backbone[:400] + _rand(rng, 30, first_not=backbone[400]) + b"N" + _rand(rng, 30, last_not=backbone[399]) + backbone[400:800])
    add("all", _rand(rng, 333))
    add("short", backbone[:k - 1])
    add("homo", b"A" * (k + 9))
    add("start_a", b"A" * (k + 10) + backbone[50:300])
    add("end_a", backbone[300:600] + b"A" * (k + 10))
    # ``edges``: EDGES_POSITIONS positions of the backbone, a whole number of tiles, with five substitutions — each makes the k
    # positions whose windows hold it novel: runs that START at positions WAVE, TILE and 2 CHUNK, a run whose last position is
    # CHUNK - 1, and a run that reaches the contig's end
    edges = _periodic(backbone[:UNIT], EDGES_POSITIONS + k - 1)
    for at in (WAVE + k - 1, TILE + k - 1, CHUNK - 1, 2 * CHUNK + k - 1, EDGES_POSITIONS - 1):
        edges = sub(edges, at)
    add("edges", edges)
    promises = dict(homo=homo, sat3=sorted(_window_keys(sat3, k)), sat11=sorted(_window_keys(long_c, k)), twice=twice, edge=edge,
                    broken=broken, lower=lower, exact=exact, held=plain[:200], del_at=del_at, runs={n: i for i, n in enumerate(names)})
    return table, [a, b], R, promises


# ---------------------------------------------------------------------------
# what tests/test_gpu_novel.py and tests/test_gpu_novel_runs.py share: the pan table loaded with the crafted keys
# ---------------------------------------------------------------------------
GPU_K = 21
GPU_MIN_COUNT = 2  # what the crafted sample's ``edge`` key straddles
GPU_WIDTHS = [8, 33, 65, 97]  # byte masks (created dense), slots, inline, split


def masks(n, nkeys, seed=0):
    """which genomes hold each key: random, no key without a bit"""
    rng = np.random.default_rng(1000 * n + seed)
    M = (rng.random((nkeys, n)) < rng.random((nkeys, 1))).astype(np.uint8)
    none = M.sum(axis=1) == 0
    M[none, rng.integers(0, n, int(none.sum()))] = 1
    return M


def load(tbl, keys, M):
    for d, words in enumerate(KR.group_words(M)):
        has = words != 0
        tbl.insert_keys(d, keys[has], words[has])


def pan_table(ctx, k, n, keys, **kw):
    from panagram_amd import engine
    tbl = engine.PanTable(ctx, k, n, **kw)
    load(tbl, keys, masks(n, len(keys)))
    assert tbl.stats()["nkeys"] == len(keys)
    return tbl


# ---------------------------------------------------------------------------
# novel end to end: the index of tests/place_ref.py (A, B, C) and a sample made from genome B
# ---------------------------------------------------------------------------
E2E_INSERTION, E2E_INS_AT, E2E_SUB_AT, E2E_DEL_AT, E2E_DEL_LEN, E2E_NOVEL_CONTIG = 500, 10000, 20000, 12000, 40, 3000
E2E_SAMPLE_NAMES = ["s1", "s2", "s3", "s4"]
E2E_READ_LEN, E2E_COVERAGE, E2E_ERRORS = 100, 8, 60


def e2e_del_at():
    from tests import place_ref as pr
    return _del_at(pr.e2e_genomes()[0][1][1], E2E_DEL_AT, E2E_DEL_LEN)


@functools.lru_cache(maxsize=None)
def e2e_sample():
    """the contigs of a FASTA sample: genome B with a planted 500-base random insertion and one substitution in its first contig,
    one deletion in its second, its third as it is, and one wholly novel contig"""
    from tests import place_ref as pr
    B = pr.e2e_genomes()[0][1]
    rng = np.random.default_rng(pr.E2E["seed"] + 7)
    c0 = B[0][:E2E_INS_AT] + _rand(rng, E2E_INSERTION, B[0][E2E_INS_AT], B[0][E2E_INS_AT - 1]) + B[0][E2E_INS_AT:]
    at = E2E_SUB_AT
    c0 = c0[:at] + bytes([b"ACGT"[(b"ACGT".index(c0[at]) + 1) % 4]]) + c0[at + 1:]
    at = e2e_del_at()
    c1 = B[1][:at] + B[1][at + E2E_DEL_LEN:]
    return [c0, c1, B[2], _rand(rng, E2E_NOVEL_CONTIG)]


@functools.lru_cache(maxsize=None)
def e2e_reads():
    """(reads, error keys): error-free reads of ``e2e_sample`` on both strands — every base covered: the reads tile each contig at a
    stride, then at random — and E2E_ERRORS reads with one substitution each, each planted ONCE at a place of its own; the keys of
    the windows that hold a planted error and that neither the index nor the error-free sample holds"""
    from tests import place_ref as pr
    k = pr.E2E["k"]
    rng = np.random.default_rng(pr.E2E["seed"] + 8)
    sample = e2e_sample()
    reads = []
    for c in sample:
        starts = list(range(0, len(c) - E2E_READ_LEN, E2E_READ_LEN // 4)) + [len(c) - E2E_READ_LEN]
        starts += [0, len(c) - E2E_READ_LEN]  # (a contig's first and last bases lie in its first and last read alone: twice)
        starts += [int(s) for s in rng.integers(0, len(c) - E2E_READ_LEN + 1, E2E_COVERAGE * len(c) // E2E_READ_LEN)]
        reads += [c[s:s + E2E_READ_LEN] for s in starts]
    clean = set(int(x) for x in cr.valid_keys(sample, k)) | set(int(x) for x in SR.e2e_table()[0])
    errors = set()
    for i in rng.choice(len(reads), E2E_ERRORS, replace=False):
        r = reads[int(i)]
        at = 25 + int(rng.integers(0, 50))
        bad = r[:at] + bytes([b"ACGT"[(b"ACGT".index(r[at]) + 1 + int(rng.integers(0, 3))) % 4]]) + r[at + 1:]
        reads.append(bad)  # (beside the read it was made from, which stays)
        errors |= _window_keys(bad, k) - clean
    reads = [r if rng.random() < 0.5 else SR.revcomp(r) for r in reads]
    return reads, errors


def e2e_model(sample, min_count, min_bases=0, file=""):
    """(stats, spectrum, kmers, regions) as Index.novel returns them with ``kmers`` and — for a FASTA sample — ``regions`` set, from
    the model's counts and panagram_amd.novel's frames.  ``sample``: "reads" — e2e_reads() — or "fasta" — e2e_sample()"""
    from panagram_amd import novel as nov
    from tests import place_ref as pr
    keys, k = SR.e2e_table()[0], pr.E2E["k"]
    if sample == "reads":
        reads = e2e_reads()[0]
        contigs, nreads, nbases, regions = pr.joined_reads(reads), len(reads), sum(len(r) for r in reads), None
    else:
        contigs = e2e_sample()
        nreads, nbases = len(contigs), sum(len(c) for c in contigs)
        rc, ra, rb, lh, rh, _, _ = runs(keys, contigs, k)
        regions = nov.filter_regions(nov.regions_frame(file, E2E_SAMPLE_NAMES, rc, ra, rb, lh, rh, k), min_bases)
    windows, hits, nk, d = novel_counts(keys, [contigs], k)
    counts = result(d, min_count)
    return (nov.stats(counts, min_count, windows, hits, nreads, nbases, regions), nov.spectrum_frame(counts["depth_hist"]),
            nov.kmers_frame(*solid_keys(nk, d, min_count), k), regions)
