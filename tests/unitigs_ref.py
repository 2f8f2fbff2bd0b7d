"""What pg_unitigs.hip computes, restated over a dict of integer keys, a second time by brute force over strings, and the crafted
sample both are held to.  No tests in here: tests/test_unitigs_cpu.py holds the model to the brute force and the crafted sample to
its promises, tests/test_gpu_unitigs.py holds the kernels to the model.  Oracle side only; never imported by the product.

Over the novel k-mers of a sample (tests/novel_ref.py: ``novel_counts``), their depths, a ``min_count`` and k (2 <= k <= 32):

  node              a solid novel key: a canonical k-mer of the novel table with depth >= min_count.  Keys below min_count and k-mers
                    the pan table holds are not nodes: they cut paths.
  oriented k-mer    w: a node's k-mer x or its reverse complement; canon(w) is its node.
  out(w)            the bases b for which canon(w[1:] + b) is a node (0 to 4 of them);  in(w) = out(rc(w)), complemented.
  link byte         of node x, in the canonical orientation (first base most significant, A < C < G < T): bit b (b < 4) is set when
                    canon(x[1:] + b) is a node, bit 4 + b when canon(b + x[:-1]) is a node.
  compactable edge  w -> w': out(w) = {the base that gives w'}, in(w') holds exactly one base, canon(w) != canon(w') (no self-loop
                    such as A..A, no hairpin w -> rc(w)), and neither node is its own reverse complement (even k only).
  unitig            a maximal path w1 .. wn along compactable edges, all nodes distinct; its sequence is w1 plus the last base of
                    each further wi: n + k - 1 bases.  A node that is its own reverse complement is a unitig of n = 1.  Every node
                    lies in exactly one unitig.
  circular unitig   a component in which every node has a compactable edge on both sides.  Emitted once, from its smallest key in
                    that key's canonical orientation, walking to the right: n nodes, n + k - 1 bases.
  linear unitig     emitted once; the smaller of its sequence and the reverse complement stands for it.
  depth_sum         the sum of the nodes' depths."""
import functools

import numpy as np

from tests import novel_ref as NR
from tests import screen_ref as SR


# ---------------------------------------------------------------------------
# the model: integer keys
# ---------------------------------------------------------------------------
def rc(w: int, k: int) -> int:
    r = 0
    for _ in range(k):
        r = (r << 2) | (3 - (w & 3))
        w >>= 2
    return r


def canon(w: int, k: int) -> int:
    return min(w, rc(w, k))


def nodes_of(nkeys, depths, min_count) -> dict:
    """{key: depth} of the solid novel keys"""
    return {int(x): int(d) for x, d in zip(np.asarray(nkeys).tolist(), np.asarray(depths).tolist()) if d >= int(min_count)}


def out_bases(w: int, nodes, k: int):
    mask = (1 << (2 * k)) - 1
    return [b for b in range(4) if canon(((w << 2) | b) & mask, k) in nodes]


def in_bases(w: int, nodes, k: int):
    return [b for b in range(4) if canon((w >> 2) | (b << (2 * (k - 1))), k) in nodes]


def link_byte(x: int, nodes, k: int) -> int:
    return sum(1 << b for b in out_bases(x, nodes, k)) | sum(16 << b for b in in_bases(x, nodes, k))


def links(nodes, k: int):
    """(the nodes' keys sorted [uint64], their link bytes [uint8])"""
    keys = sorted(nodes)
    return np.array(keys, np.uint64), np.array([link_byte(x, nodes, k) for x in keys], np.uint8)


def step(w: int, nodes, k: int):
    """the oriented k-mer behind the compactable edge out of w, or None"""
    if rc(w, k) == w:
        return None
    out = out_bases(w, nodes, k)
    if len(out) != 1:
        return None
    w2 = ((w << 2) | out[0]) & ((1 << (2 * k)) - 1)
    if rc(w2, k) == w2 or canon(w2, k) == canon(w, k) or len(in_bases(w2, nodes, k)) != 1:
        return None
    return w2


def spell(w: int, k: int) -> str:
    return "".join("ACGT"[(w >> (2 * (k - 1 - i))) & 3] for i in range(k))


def revcomp(seq: str) -> str:
    return seq.translate(str.maketrans("ACGT", "TGCA"))[::-1]


def path_sequence(path, k: int) -> str:
    return spell(path[0], k) + "".join("ACGT"[w & 3] for w in path[1:])


def unitig_paths(nodes, k: int):
    """[(path of oriented k-mers, circular)], every node in exactly one path.  A linear path comes in the orientation that starts
    at the end with the smaller key (n = 1: the canonical one), a circular one from its smallest key in the canonical orientation."""
    seen, out = set(), []
    for x in sorted(nodes):
        if x in seen:
            continue
        # to the left end: the edge u -> w is compactable iff rc(w) -> rc(u) is
        w, circular = x, False
        while True:
            u = step(rc(w, k), nodes, k)
            if u is None:
                break
            w = rc(u, k)
            if w == x:
                circular = True
                break
        path = [w]
        while True:
            w2 = step(path[-1], nodes, k)
            if w2 is None or w2 == path[0]:
                break
            path.append(w2)
        if circular:  # (sorted: x is the cycle's smallest key, in its canonical orientation)
            assert path[0] == x and step(path[-1], nodes, k) == x
        elif len(path) > 1 and canon(path[-1], k) < canon(path[0], k):
            path = [rc(w, k) for w in reversed(path)]
        elif len(path) == 1:
            path = [x]
        members = [canon(w, k) for w in path]
        assert not seen & set(members) and len(set(members)) == len(members)
        seen.update(members)
        out.append((path, circular))
    assert seen == set(nodes)
    return out


def unitigs(nodes, k: int):
    """the set of (sequence, kmers, depth_sum, circular): a linear sequence as the smaller of itself and its reverse complement, a
    circular one from its smallest key in that key's canonical orientation"""
    out = set()
    for path, circular in unitig_paths(nodes, k):
        seq = path_sequence(path, k)
        out.add((seq if circular else min(seq, revcomp(seq)), len(path), sum(nodes[canon(w, k)] for w in path), int(circular)))
    return out


def check_partition(unitig_set, nodes, k: int):
    """the canonical k-mers of all unitig sequences are the nodes, each once; the depths add up"""
    got = []
    for seq, n, dsum, _ in unitig_set:
        assert len(seq) == n + k - 1, (seq, n)
        mers = [brute_canon(seq[i:i + k]) for i in range(n)]
        assert sum(nodes[int(m.translate(_DIGITS), 4)] for m in mers) == dsum, seq
        got += mers
    assert len(got) == len(set(got)) == len(nodes)
    assert set(int(m.translate(_DIGITS), 4) for m in got) == set(nodes)


def check_maximal(unitig_set, nodes, k: int):
    """no compactable edge leaves a linear unitig at either end; the one out of a circular unitig's last node leads to its first"""
    for seq, n, _, circular in unitig_set:
        first, last = int(seq[:k].translate(_DIGITS), 4), int(seq[n - 1:n - 1 + k].translate(_DIGITS), 4)
        if circular:
            assert step(last, nodes, k) == first and first == min(canon(int(seq[i:i + k].translate(_DIGITS), 4), k) for i in range(n)), seq
        else:
            assert step(last, nodes, k) is None and step(rc(first, k), nodes, k) is None, seq
        for i in range(n - 1):  # and every edge inside is one
            assert step(int(seq[i:i + k].translate(_DIGITS), 4), nodes, k) == int(seq[i + 1:i + 1 + k].translate(_DIGITS), 4), (seq, i)


# ---------------------------------------------------------------------------
# brute force: strings, with a reverse complement and a canonical form of its own
# ---------------------------------------------------------------------------
_DIGITS = str.maketrans("ACGT", "0123")
_PAIR = {"A": "T", "C": "G", "G": "C", "T": "A"}


def brute_rc(s: str) -> str:
    return "".join(_PAIR[ch] for ch in reversed(s))


def brute_canon(s: str) -> str:
    r = brute_rc(s)
    return s if s <= r else r


def brute_nodes(table_keys, sets, k: int, min_count: int) -> dict:
    """{canonical k-mer string: depth} of the sample's solid k-mers that the table does not hold, by a walk over every window"""
    held = set(SR.spell(int(x), k).decode() for x in table_keys)
    depth = {}
    for contigs in sets:
        for seq in contigs:
            seq = bytes(seq).decode().upper()
            for p in range(len(seq) - k + 1):
                w = seq[p:p + k]
                if set(w) <= set("ACGT"):
                    c = brute_canon(w)
                    if c not in held:
                        depth[c] = depth.get(c, 0) + 1
    return {c: d for c, d in depth.items() if d >= min_count}


def brute_unitigs(nodes: dict):
    """the same set as ``unitigs`` from {canonical k-mer string: depth}: every compactable edge between oriented k-mers listed
    first, the paths then read off the edge list"""
    oriented = set(nodes) | set(brute_rc(s) for s in nodes)

    def succ(w):
        return [w[1:] + b for b in "ACGT" if w[1:] + b in oriented]

    def pred(w):
        return [b + w[:-1] for b in "ACGT" if b + w[:-1] in oriented]
    nxt, prv = {}, {}
    for w in oriented:
        s = succ(w)
        if len(s) == 1 and len(pred(s[0])) == 1 and brute_canon(w) != brute_canon(s[0]) and w != brute_rc(w) and s[0] != brute_rc(s[0]):
            nxt[w] = s[0]
            prv[s[0]] = w
    out, done = set(), set()

    def emit(path, circular):
        seq = path[0] + "".join(w[-1] for w in path[1:])
        done.update(brute_canon(w) for w in path)
        out.add((seq if circular else min(seq, brute_rc(seq)), len(path), sum(nodes[brute_canon(w)] for w in path), int(circular)))
    for w in sorted(oriented):
        if w in prv or brute_canon(w) in done:
            continue
        path = [w]
        while path[-1] in nxt:
            path.append(nxt[path[-1]])
        emit(path, False)
    for c in sorted(nodes):  # what is left lies on cycles: from the smallest key of each, as it is spelled canonically
        if c in done:
            continue
        path = [c]
        while nxt[path[-1]] != c:
            path.append(nxt[path[-1]])
        emit(path, True)
    return out


def strings_of(nodes: dict, k: int) -> dict:
    return {spell(x, k): d for x, d in nodes.items()}


# ---------------------------------------------------------------------------
# seeded random graphs at small k: palindromes, hairpins, satellites and cycles among them
# ---------------------------------------------------------------------------
def random_graph(seed: int) -> tuple:
    """(k, {key: depth}): canonical k-mers of random walks, random circles and a random sprinkle, k = 3 to 9"""
    rng = np.random.default_rng(seed)
    k = 3 + seed % 7
    text = []
    for _ in range(int(rng.integers(1, 6))):
        text.append("".join("ACGT"[i] for i in rng.integers(0, 4, int(rng.integers(k, 6 * k)))))
    for _ in range(int(rng.integers(0, 4))):  # circles, periods below and above k
        z = "".join("ACGT"[i] for i in rng.integers(0, 4, int(rng.integers(1, 3 * k))))
        text.append((z * (k // len(z) + 2))[:len(z) + k - 1])
    if rng.random() < 0.3:
        text.append("A" * (k + 2))
    nodes = {}
    for s in text:
        for p in range(len(s) - k + 1):
            w = int(s[p:p + k].translate(_DIGITS), 4)
            nodes[canon(w, k)] = nodes.get(canon(w, k), 0) + 1
    if seed % 3 == 0:  # (a sprinkle of chance neighbours: branches everywhere; without it the circles stay circles)
        for x in rng.integers(0, 4 ** k, int(rng.integers(0, 4 ** k // 8 + 2))).tolist():
            nodes.setdefault(canon(int(x), k), 1)
    return k, nodes


# ---------------------------------------------------------------------------
# the crafted table and the crafted sample
# ---------------------------------------------------------------------------
KS = [6, 21, 31, 32]
MIN_COUNT = 2                # what the crafted sample is built around; the tests ask at 1, 2 and 3 from one table
EXACT_FROM_K = NR.EXACT_FROM_K
INSERTION = NR.INSERTION
LONG_KMERS = 5000
CIRCLE = 300                 # k-mers of the circular sequence: more than one block's 256 lanes
ENTRY_CIRCLE = 40
SHORT_CONTIGS = 3000
SCAN_SLOTS = 4096            # slots of one block of the scan over a small table


def _seq(rng, n, first_not=None, last_not=None) -> bytes:
    return NR._rand(rng, n, first_not, last_not)


@functools.lru_cache(maxsize=None)
def crafted(k, seed=0):
    """(table keys, [set a, set b], promises) — left alone by every test that shares it.

    The table: every k-mer of a random backbone, and the one k-mer ``held`` of the middle of an otherwise novel contig.  The sample:
    every piece below once in set a and once, on a random strand, in set b (depth 2 = MIN_COUNT), unless it says otherwise.
    promises: name -> what the piece promises at MIN_COUNT (sequences as ``unitigs`` gives them), exact from EXACT_FROM_K on.

      isolated   a contig of exactly k bases: n = 1
      insertion  INSERTION bases in a held backbone, in set b reverse-complemented: ONE unitig of INSERTION + k - 1 k-mers, the
                 contig's slice; the other strand adds none
      long       a novel contig of LONG_KMERS k-mers: one lane, thousands of steps
      bubble     two alleles of one contig: left flank, two arms of k k-mers, right flank; the branch nodes have two out-bits
      tip        a dead-end branch of 5 k-mers off a contig: a unitig of its own
      below      a contig whose middle k-mer is seen MIN_COUNT - 1 times: two unitigs at MIN_COUNT, one at MIN_COUNT - 1
      held       a contig whose middle k-mer the table holds: two unitigs
      homo       a run of k + 5 A: a self-loop, the A..A node is a unitig of 1
      hairpin    (odd k) a path into w -> rc(w): ends at w
      palindrome (even k) a node that is its own reverse complement inside a path: a unitig of 1
      sat3, sat11  novel_ref's satellites: circular unitigs of 3 and 11 nodes
      circle     a circular sequence of CIRCLE k-mers
      entry      a path leading into a cycle of ENTRY_CIRCLE: not circular, cut at the branch
      short      SHORT_CONTIGS contigs of 3 k-mers: solid keys in many scan blocks
      deep       a contig seen three times; once  contigs of set a alone (depth 1)"""
    rng = np.random.default_rng(7000 * k + seed)
    while True:  # (k = 6: the backbone may hold the homopolymer or a satellite's key by chance; the next one)
        backbone = NR._periodic(_seq(rng, NR.UNIT), 1200)
        bkeys = NR._window_keys(backbone, k)
        sat3 = NR._periodic(NR.SAT3, 60 + k)
        sat11 = NR._periodic(NR.SAT11, 80 + k)
        reserved = {SR.canonical(b"A" * k, k)} | NR._window_keys(sat3, k) | NR._window_keys(sat11, k)
        if not bkeys & reserved:
            break
    P = {}
    a, b = [], []

    def both(seq, times=2):
        a.append(seq)
        for _ in range(times - 1):
            b.append(seq if rng.random() < 0.5 else SR.revcomp(seq))
        return seq

    def canon_text(seq: bytes) -> str:
        s = seq.decode()
        return min(s, revcomp(s))
    P["isolated"] = canon_text(both(_seq(rng, k)))
    ins = backbone[:500] + _seq(rng, INSERTION, backbone[500], backbone[499]) + backbone[500:1000]
    a.append(ins)
    b.append(SR.revcomp(ins))
    P["insertion"] = (canon_text(ins[500 - k + 1:500 + INSERTION + k - 1]), INSERTION + k - 1)
    P["long"] = canon_text(both(_seq(rng, LONG_KMERS + k - 1)))
    # the bubble: the alleles differ at base m
    m, flank = 3 * k, _seq(rng, 6 * k + 1)
    other = bytes([b"ACGT"[(b"ACGT".index(flank[m]) + 1 + int(rng.integers(0, 3))) % 4]])
    alt = flank[:m] + other + flank[m + 1:]
    both(flank)
    both(alt)
    P["bubble"] = dict(left=canon_text(flank[:m]), right=canon_text(flank[m + 1:]), arms={canon_text(flank[m - k + 1:m + k]), canon_text(alt[m - k + 1:m + k])},
                       branch=(SR.canonical(flank[m - k:m], k), SR.canonical(flank[m + 1:m + 1 + k], k)))
    # the tip: off the k-mer at position k of a contig of 4 k bases
    trunk = both(_seq(rng, 4 * k))
    tip = both(trunk[k:2 * k] + bytes([b"ACGT"[(b"ACGT".index(trunk[2 * k]) + 1) % 4]]) + _seq(rng, 4))
    P["tip"] = dict(tip=canon_text(tip[1:]), before=canon_text(trunk[:2 * k]), after=canon_text(trunk[k + 1:]))
    # a node below MIN_COUNT in the middle of a path of 40 k-mers
    path = _seq(rng, 40 + k - 1)
    j = 17
    a.append(path)
    b.extend([path[:j + k - 1], SR.revcomp(path[j + 1:])])
    P["below"] = dict(whole=canon_text(path), parts={canon_text(path[:j + k - 1]), canon_text(path[j + 1:])}, key=SR.canonical(path[j:j + k], k))
    # a held k-mer in the middle of a novel path
    cut = both(_seq(rng, 30 + k - 1))
    held = SR.canonical(cut[12:12 + k], k)
    P["held"] = dict(parts={canon_text(cut[:12 + k - 1]), canon_text(cut[13:])}, key=held)
    both(b"A" * (k + 5))
    P["homo"] = "A" * k
    if k % 2:
        half = _seq(rng, (k - 1) // 2)
        s = half + SR.revcomp(half)
        lead = _seq(rng, k + 1, last_not=None)
        P["hairpin"] = canon_text(both(lead + s))  # (its last window w = lead[-1] + s, and s + complement(lead[-1]) is rc(w))
    else:
        half = _seq(rng, k // 2)
        pal = half + SR.revcomp(half)
        both(_seq(rng, k) + pal + _seq(rng, k))
        P["palindrome"] = pal.decode()
    both(sat3, 3)
    both(sat11, 3)
    P["sat3"], P["sat11"] = sorted(NR._window_keys(sat3, k)), sorted(NR._window_keys(sat11, k))
    z = _seq(rng, CIRCLE)
    both(z + z[:k - 1])
    P["circle"] = z.decode()
    z2 = _seq(rng, ENTRY_CIRCLE)
    entry = _seq(rng, k + 5, last_not=z2[-1])
    both(entry + z2 + z2[:k])  # (the cycle's first k-mer a second time: the closing edge is spelled)
    P["entry"] = dict(path=canon_text((entry + z2[:k - 1])), cycle=canon_text(z2 + z2[:k - 1]))
    for _ in range(SHORT_CONTIGS):
        both(_seq(rng, k + 2))
    P["deep"] = canon_text(both(_seq(rng, 25 + k - 1), 3))
    P["once"] = [canon_text(s) for s in (_seq(rng, 10 + k - 1) for _ in range(20))]
    a.extend(s.encode() for s in P["once"])
    table = np.array(sorted(bkeys | {held}), np.uint64)
    return table, [a, b], P


@functools.lru_cache(maxsize=None)
def crafted_counts(k):
    """(the model after set a, after both): novel_ref.novel_counts' (windows, hits, novel keys, depths)"""
    table, sets, _ = crafted(k)
    return NR.novel_counts(table, sets[:1], k), NR.novel_counts(table, sets, k)


@functools.lru_cache(maxsize=None)
def crafted_model(k, min_count):
    """(nodes, link keys, link bytes, unitig set) of the crafted sample at ``min_count`` — computed once, left alone"""
    _, _, nk, d = crafted_counts(k)[1]
    nodes = nodes_of(nk, d, min_count)
    lk, lb = links(nodes, k)
    return nodes, lk, lb, unitigs(nodes, k)


def unpack(arrays: dict, k: int):
    """``engine.NovelTable.unitigs``' arrays as the model's set; a circular sequence as it came"""
    text = np.asarray(arrays["bases"], np.uint8).tobytes().decode("ascii")
    out = []
    for o, n, ds, c in zip(arrays["offsets"].tolist(), arrays["kmers"].tolist(), arrays["depth_sum"].tolist(), arrays["circular"].tolist()):
        seq = text[o:o + n + k - 1]
        out.append((seq if c else min(seq, revcomp(seq)), n, ds, c))
    return out


def e2e_insertion() -> str:
    """the insertion planted into novel_ref's end-to-end sample with the k - 1 bases on either side: its novel region's slice"""
    from tests import place_ref as pr
    k, c0 = pr.E2E["k"], NR.e2e_sample()[0]
    s = c0[NR.E2E_INS_AT - k + 1:NR.E2E_INS_AT + NR.E2E_INSERTION + k - 1].decode()
    return min(s, revcomp(s))
