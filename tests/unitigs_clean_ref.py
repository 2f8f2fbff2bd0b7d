"""What k_unitig_clean of pg_unitigs.hip and pg_novel_clean compute — error tips clipped and bubbles popped before the solid novel
k-mers are compacted — restated over a dict of integer keys, a second time by brute force over strings, with the seeded random
graphs and the crafted sample both are held to.  No tests in here: tests/test_unitigs_clean_cpu.py holds the model to the brute
force and the crafted cases to their promises, tests/test_gpu_unitigs_clean.py holds the kernels to the model.  Oracle side only.

The vocabulary is tests/unitigs_ref.py's (node, oriented k-mer, out, in, compactable edge, linear unitig U = w1 .. wn).  Over the
graph G of the current nodes, with tip_kmers T, bubble_kmers B (1 to 1024, default 2 k), a ratio Rm in per mille (1 to 999, default
250) and rounds (0 to 64, default 4):

  side        the right side of U is out(wn), the left side in(w1).  A side is DEAD when that set is empty, ATTACHED BY v when the
              set holds exactly one base and the oriented k-mer v it names (wn[1:] + b on the right, b + w1[:-1] on the left) is a
              node that is none of U's nodes on either strand and not its own reverse complement; every other side is open.
  tip         U is linear with n <= T, one side dead, the other attached by v.  S = the other oriented k-mers with an edge into v on
              that side (right side: the predecessors of v but wn; left side: the successors of v but w1), none left out.  U is
              clipped iff S is not empty and depth(attached end node) * 1000 <= Rm * max over S of depth(s).
  bubble      U is linear with n <= B, its left side attached by p, its right side by q.  A parallel U' is another linear unitig
              of n' <= B nodes whose left side is attached by the same oriented p and whose right side by the same oriented q — the
              unitig that starts at a successor s != w1 of p with in(s) = {p's base}, walked to the right.  (The left side of U' is
              asked for as its right side is: so the rule reads the same from either end of U.)  With e(X) = min(depth of X's two
              end nodes), U is popped iff some parallel U' has e(U) * 1000 <= Rm * e(U').  p = q is nothing special.
  rounds      Jacobi: every decision of round r is taken on G_r, D_r is what it drops, G_{r+1} = G_r minus D_r.  The rounds stop
              at the first empty D_r or after ``rounds`` of them; ``rounds run`` counts those that dropped something.
A circular unitig, a unitig dead on both sides and a unitig of one palindromic node are never dropped (no side of the last is
attached or dead in a way that matters: it has n = 1 and is tested like any other)."""
import functools

import numpy as np

from tests import novel_ref as NR
from tests import screen_ref as SR
from tests import unitigs_ref as UR

RATIO_MILLI = 250
ROUNDS = 4
STAT_NAMES = ["clipped_tips", "clipped_kmers", "popped_bubbles", "popped_kmers", "clean_rounds"]


def default_kmers(k: int) -> int:
    return 2 * k


# ---------------------------------------------------------------------------
# the model: integer keys
# ---------------------------------------------------------------------------
def flip(path, k):
    return [UR.rc(w, k) for w in reversed(path)]


def right_side(path, nodes, k):
    """("dead", None), ("att", v) or ("open", None) of the right side of the oriented path"""
    out = UR.out_bases(path[-1], nodes, k)
    if not out:
        return "dead", None
    if len(out) == 1:
        v = ((path[-1] << 2) | out[0]) & ((1 << (2 * k)) - 1)
        if UR.rc(v, k) != v and UR.canon(v, k) not in set(UR.canon(w, k) for w in path):
            return "att", v
    return "open", None


def preds(v, nodes, k):
    return [(v >> 2) | (b << (2 * (k - 1))) for b in UR.in_bases(v, nodes, k)]


def succs(p, nodes, k):
    return [((p << 2) | b) & ((1 << (2 * k)) - 1) for b in UR.out_bases(p, nodes, k)]


def walk_right(s, nodes, k, limit):
    """the path from s along compactable edges to its end, None when it holds more than ``limit`` nodes"""
    path = [s]
    while True:
        w2 = UR.step(path[-1], nodes, k)
        if w2 is None:
            return path
        if len(path) == limit:
            return None
        path.append(w2)


def is_tip(path, nodes, k, T, Rm):
    if len(path) > T:
        return False
    for P in (path, flip(path, k)):
        kind, v = right_side(P, nodes, k)
        if kind != "att" or right_side(flip(P, k), nodes, k)[0] != "dead":
            continue
        S = [s for s in preds(v, nodes, k) if s != P[-1]]
        if S and nodes[UR.canon(P[-1], k)] * 1000 <= Rm * max(nodes[UR.canon(s, k)] for s in S):
            return True
    return False


def e_of(path, nodes, k):
    return min(nodes[UR.canon(path[0], k)], nodes[UR.canon(path[-1], k)])


def is_bubble(path, nodes, k, B, Rm):
    if len(path) > B:
        return False
    kr, q = right_side(path, nodes, k)
    kl, rp = right_side(flip(path, k), nodes, k)
    if kr != "att" or kl != "att":
        return False
    p = UR.rc(rp, k)
    for s in succs(p, nodes, k):
        if s == path[0] or len(UR.in_bases(s, nodes, k)) != 1:
            continue
        other = walk_right(s, nodes, k, B)
        if other is None or right_side(other, nodes, k) != ("att", q) or right_side(flip(other, k), nodes, k) != ("att", rp):
            continue
        if e_of(path, nodes, k) * 1000 <= Rm * e_of(other, nodes, k):
            return True
    return False


def clean_round(nodes, k, T, B, Rm):
    """(the keys round drops, [tips, their nodes, bubbles, their nodes]) on the graph of ``nodes``"""
    drop, st = set(), [0, 0, 0, 0]
    for path, circular in UR.unitig_paths(nodes, k):
        if circular:
            continue
        if is_tip(path, nodes, k, T, Rm):
            st[0] += 1
            st[1] += len(path)
        elif is_bubble(path, nodes, k, B, Rm):
            st[2] += 1
            st[3] += len(path)
        else:
            continue
        drop.update(UR.canon(w, k) for w in path)
    return drop, st


def clean(nodes, k, T=None, B=None, Rm=RATIO_MILLI, rounds=ROUNDS, trace=None):
    """(the surviving {key: depth}, {STAT_NAMES}); trace: a list that takes every round's dropped keys"""
    T = default_kmers(k) if T is None else T
    B = default_kmers(k) if B is None else B
    nodes, total, run = dict(nodes), [0, 0, 0, 0], 0
    for _ in range(rounds):
        drop, st = clean_round(nodes, k, T, B, Rm)
        if not drop:
            break
        if trace is not None:
            trace.append(drop)
        run += 1
        total = [a + b for a, b in zip(total, st)]
        nodes = {x: d for x, d in nodes.items() if x not in drop}
    return nodes, dict(zip(STAT_NAMES, total + [run]))


# ---------------------------------------------------------------------------
# brute force: strings.  Every oriented linear unitig listed from the edge list, both ways round; a bubble's parallels are found by
# searching that list for the same (p, q), not by walking from p
# ---------------------------------------------------------------------------
def brute_round(nodes: dict, T, B, Rm):
    """the canonical strings the round drops and [tips, their nodes, bubbles, their nodes], from {canonical k-mer string: depth}"""
    rcs, can = UR.brute_rc, UR.brute_canon
    oriented = set(nodes) | set(rcs(s) for s in nodes)

    def succ(w):
        return [w[1:] + b for b in "ACGT" if w[1:] + b in oriented]

    def pred(w):
        return [b + w[:-1] for b in "ACGT" if b + w[:-1] in oriented]
    nxt, prv = {}, {}
    for w in oriented:
        s = succ(w)
        if len(s) == 1 and len(pred(s[0])) == 1 and can(w) != can(s[0]) and w != rcs(w) and s[0] != rcs(s[0]):
            nxt[w] = s[0]
            prv[s[0]] = w
    paths = []
    for w in sorted(oriented):
        if w in prv:
            continue
        path = [w]
        while path[-1] in nxt:
            path.append(nxt[path[-1]])
        paths.append(path)

    def attached(side, members):
        return len(side) == 1 and side[0] != rcs(side[0]) and can(side[0]) not in members
    ends = {}
    for P in paths:
        members = set(can(w) for w in P)
        L, R = pred(P[0]), succ(P[-1])
        if len(P) <= B and attached(L, members) and attached(R, members):
            ends.setdefault((L[0], R[0]), []).append(P)
    drop, tips, bubbles = set(), set(), set()
    for P in paths:
        members = frozenset(can(w) for w in P)
        L, R = pred(P[0]), succ(P[-1])
        if len(P) <= T and not L and attached(R, members):
            S = [s for s in pred(R[0]) if s != P[-1]]
            if S and nodes[can(P[-1])] * 1000 <= Rm * max(nodes[can(s)] for s in S):
                tips.add(members)
    for (p, q), group in ends.items():
        for P in group:
            e = min(nodes[can(P[0])], nodes[can(P[-1])])
            if any(Q is not P and e * 1000 <= Rm * min(nodes[can(Q[0])], nodes[can(Q[-1])]) for Q in group):
                bubbles.add(frozenset(can(w) for w in P))
    for m in tips | bubbles:
        drop |= m
    return drop, [len(tips), sum(len(m) for m in tips), len(bubbles), sum(len(m) for m in bubbles)]


def brute_clean(nodes: dict, T, B, Rm=RATIO_MILLI, rounds=ROUNDS):
    nodes, total, run = dict(nodes), [0, 0, 0, 0], 0
    for _ in range(rounds):
        drop, st = brute_round(nodes, T, B, Rm)
        if not drop:
            break
        run += 1
        total = [a + b for a, b in zip(total, st)]
        nodes = {x: d for x, d in nodes.items() if x not in drop}
    return nodes, dict(zip(STAT_NAMES, total + [run]))


# ---------------------------------------------------------------------------
# seeded random graphs at k = 3 to 9: a few deep sequences and circles, and shallow copies of pieces of them with one base changed
# in the middle (a bubble), near an end (a tip) or both
# ---------------------------------------------------------------------------
def random_graph(seed: int):
    """(k, {key: depth}, T, B, Rm): depths 10 to 30 along the true sequences, 1 to 3 along the erroneous copies"""
    rng = np.random.default_rng(90000 + seed)
    k = 3 + seed % 7
    deep, shallow = [], []
    for _ in range(int(rng.integers(1, 4))):
        deep.append("".join("ACGT"[i] for i in rng.integers(0, 4, int(rng.integers(3 * k, 9 * k)))))
    if rng.random() < 0.4:  # a circle
        z = "".join("ACGT"[i] for i in rng.integers(0, 4, int(rng.integers(k, 4 * k))))
        deep.append(z + z[:k - 1])
    for _ in range(int(rng.integers(1, 7))):
        src = deep[int(rng.integers(0, len(deep)))]
        n = int(rng.integers(k + 1, 3 * k + 2))
        at = int(rng.integers(0, max(1, len(src) - n)))
        piece = list(src[at:at + n])
        for _ in range(int(rng.integers(1, 3))):
            j = int(rng.integers(0, len(piece)))
            piece[j] = "ACGT"[("ACGT".index(piece[j]) + 1 + int(rng.integers(0, 3))) % 4]
        if rng.random() < 0.2:  # an indel
            j = int(rng.integers(1, len(piece)))
            piece[j:j] = list("ACGT"[int(rng.integers(0, 4))] * int(rng.integers(1, 4)))
        shallow.append("".join(piece))
    if rng.random() < 0.2:
        shallow.append("".join("ACGT"[i] for i in rng.integers(0, 4, k + 3)))  # stands alone
    nodes = {}
    for texts, lo, hi in ((deep, 10, 31), (shallow, 1, 4)):
        for s in texts:
            d = int(rng.integers(lo, hi))
            for p in range(len(s) - k + 1):
                x = UR.canon(int(s[p:p + k].translate(UR._DIGITS), 4), k)
                nodes[x] = nodes.get(x, 0) + d
    T, B = [(2 * k, 2 * k), (k, 2 * k), (3, k + 1), (2 * k, 2)][int(rng.integers(0, 4))]
    return k, nodes, T, B, [250, 250, 100, 500][int(rng.integers(0, 4))]


# ---------------------------------------------------------------------------
# the crafted table and sample
# ---------------------------------------------------------------------------
KS = UR.KS
MIN_COUNT = 2
EXACT_FROM_K = UR.EXACT_FROM_K
CIRCLE = 300
DEEP, WEAK = 20, 2


def _seq(rng, n, first_not=None, last_not=None) -> bytes:
    return NR._rand(rng, n, first_not, last_not)


def _other(rng, base: int) -> bytes:
    return bytes([b"ACGT"[(b"ACGT".index(base) + 1 + int(rng.integers(0, 3))) % 4]])


def _text(seq: bytes) -> str:
    s = seq.decode()
    return min(s, UR.revcomp(s))


@functools.lru_cache(maxsize=None)
def crafted(k, seed=0):
    """(table keys, sets, promises) — left alone by every test that shares it.  With T = B = 2 k, Rm = 250, min_count 2.

    Every case is planted twice from fresh random bases: once as it is built and once with every read reverse-complemented.  A
    sequence of depth d is d reads, one in each of the last d sets (the table grows between the adds; the novel table reserves slots for the windows of an add: many
    small adds keep it at a few thousand keys in 2^12 to 2^16 slots).  promises: a list of (case, kind, sequence or keys):
      ("one", text)      text (the smaller of itself and its reverse complement) is ONE linear unitig of the cleaned graph and is
                         none of the raw graph
      ("stays", keys)    every one of these keys is a node of the cleaned graph
      ("gone", keys)     none of them is
      ("circle", bases)  a circular unitig of that many k-mers stands in the cleaned graph and not in the raw one
    exact from EXACT_FROM_K on.  The cases (case names as in the list):
      tip            a dead-end branch of T nodes and depth 2 off a trunk of depth 20: clipped, the trunk one unitig
      tip_long       the same with T + 1 nodes: stays
      tip_ratio      a tip of depth 6 beside 20: above the ratio, stays
      two_ends       two dead branches at a path's end, depths 15 and 3: the shallower is clipped, path + deeper one unitig
      held_sibling   a tip that joins a trunk behind a k-mer the table holds: no sibling that is a node, stays
      isolated       a unitig of 5 nodes on its own: stays
      snp            a bubble of k and k nodes at depths 2 and 30: popped, flank + arm + flank one unitig
      even           a bubble at depths 15 and 15: both arms stay
      indel          arms of k - 1 (depth 2) and k + 3 (depth 30) nodes: the shorter is popped
      arm_long       a weak arm of B + 1 nodes: stays
      tip_on_arm     a tip of depth 2 on a bubble's arm of depth 8 beside an arm of depth 40: two rounds; open at rounds = 1
      circle         a circle of CIRCLE k-mers with a tip: circular = 1 once the tip is clipped
      odd_ends       even k: a tip that runs into a palindromic node of the trunk; odd k: a tip beside a hairpin at a trunk's end.
                     The trunk's nodes stay"""
    rng = np.random.default_rng(9100 * k + seed)
    T = B = default_kmers(k)
    backbone = _seq(rng, 300 + k - 1)
    held_keys = set(NR._window_keys(backbone, k))
    planted, P = [], []

    def keys_of(seq):
        return sorted(NR._window_keys(seq, k))
    for strand in (0, 1):
        def put(seq, depth):
            planted.append((SR.revcomp(seq) if strand else seq, depth))
            return seq
        # tip, tip_long, tip_ratio: the branch leaves the trunk to the right behind trunk[j : j + k - 1]
        for name, n, depth in (("tip", T, WEAK), ("tip_long", T + 1, WEAK), ("tip_ratio", T, 6)):
            trunk = put(_seq(rng, 6 * k), DEEP)
            j = 2 * k
            tip = put(trunk[j:j + k - 1] + _other(rng, trunk[j + k - 1]) + _seq(rng, n - 1), depth)
            if name == "tip":
                P += [(name, "one", _text(trunk)), (name, "gone", keys_of(tip))]
            else:
                P += [(name, "stays", keys_of(tip))]
        trunk = put(_seq(rng, 3 * k), DEEP)
        first = _seq(rng, 1)
        deeper = put(trunk[-(k - 1):] + first + _seq(rng, 4), 15)
        shallower = put(trunk[-(k - 1):] + _other(rng, first[0]) + _seq(rng, 4), 3)
        P += [("two_ends", "one", _text(trunk + deeper[k - 1:])), ("two_ends", "gone", keys_of(shallower))]
        # held_sibling: the trunk's k-mer at j is the table's; the tip runs into the k-mer at j + 1
        trunk = put(_seq(rng, 6 * k), DEEP)
        j = 2 * k
        held_keys |= NR._window_keys(trunk[j:j + k], k)
        tip = put(_seq(rng, T - 1) + _other(rng, trunk[j]) + trunk[j + 1:j + k], WEAK)
        P += [("held_sibling", "stays", keys_of(tip))]
        P += [("isolated", "stays", keys_of(put(_seq(rng, 5 + k - 1), WEAK)))]
        # snp, even
        for name, d0, d1 in (("snp", 30, WEAK), ("even", 15, 15)):
            m, flank = 3 * k, _seq(rng, 6 * k + 1)
            alt = flank[:m] + _other(rng, flank[m]) + flank[m + 1:]
            put(flank, d0)
            put(alt, d1)
            if name == "snp":
                P += [(name, "one", _text(flank)), (name, "gone", keys_of(alt[m - k + 1:m + k]))]
            else:
                P += [(name, "stays", keys_of(alt[m - k + 1:m + k]) + keys_of(flank[m - k + 1:m + k]))]
        # indel, arm_long: left + right against left + ins + right
        for name, nins, d_short, d_long in (("indel", 4, WEAK, 30), ("arm_long", B + 1 - (k - 1), 30, WEAK)):
            left, right = _seq(rng, 3 * k), _seq(rng, 3 * k)
            ins = _seq(rng, nins, right[0], left[-1])
            put(left + right, d_short)
            put(left + ins + right, d_long)
            junction = (left + right)[3 * k - k + 1:3 * k + k - 1]
            arm = (left + ins + right)[3 * k - k + 1:3 * k + nins + k - 1]
            if name == "indel":
                P += [(name, "one", _text(left + ins + right)), (name, "gone", keys_of(junction))]
            else:
                P += [(name, "stays", keys_of(junction) + keys_of(arm))]
        # tip_on_arm
        m, flank = 3 * k, _seq(rng, 6 * k + 1)
        alt = flank[:m] + _other(rng, flank[m]) + flank[m + 1:]
        put(flank, 40)
        put(alt, 8)
        j = m - 2  # the tip leaves the weak arm behind alt[j : j + k - 1], which holds the changed base
        tip = put(alt[j:j + k - 1] + _other(rng, alt[j + k - 1]) + _seq(rng, 3), WEAK)
        P += [("tip_on_arm", "one", _text(flank)), ("tip_on_arm", "gone", keys_of(tip) + keys_of(alt[m - k + 1:m + k]))]
        # circle
        z = _seq(rng, CIRCLE)
        put(z + z[:k - 1], DEEP)
        tip = put(z[50:50 + k - 1] + _other(rng, z[50 + k - 1]) + _seq(rng, 3), WEAK)
        P += [("circle", "circle", CIRCLE), ("circle", "gone", keys_of(tip))]
        # odd_ends
        if k % 2 == 0:
            half = _seq(rng, k // 2)
            pal = half + SR.revcomp(half)
            r1 = _seq(rng, 2 * k)
            trunk = put(r1 + pal + _seq(rng, 2 * k), DEEP)
            put(_seq(rng, 4) + _other(rng, r1[-1]) + pal[:k - 1], WEAK)
        else:
            half = _seq(rng, (k - 1) // 2)
            s = half + SR.revcomp(half)
            lead = _seq(rng, 2 * k)
            trunk = put(lead + s, DEEP)
            put(_seq(rng, 4) + _other(rng, lead[-1]) + s, WEAK)
        P += [("odd_ends", "stays", keys_of(trunk))]
    table = np.array(sorted(held_keys), np.uint64)
    return table, [[s for s, d in planted if d > i] for i in reversed(range(max(d for _, d in planted)))], P


@functools.lru_cache(maxsize=None)
def crafted_nodes(k, min_count=MIN_COUNT):
    """the raw graph's {key: depth} of the crafted sample — computed once, left alone"""
    table, sets, _ = crafted(k)
    _, _, nk, d = NR.novel_counts(table, sets, k)
    return UR.nodes_of(nk, d, min_count)


@functools.lru_cache(maxsize=None)
def crafted_model(k, rounds=ROUNDS, min_count=MIN_COUNT):
    """(surviving nodes, stats, link keys, link bytes, unitig set) of the crafted sample cleaned with the defaults"""
    nodes, st = clean(crafted_nodes(k, min_count), k, rounds=rounds)
    lk, lb = UR.links(nodes, k)
    return nodes, st, lk, lb, UR.unitigs(nodes, k)
