"""CPU: the numpy model of the synteny blocks (tests/blocks_ref.py) on cases whose blocks follow by construction, its promises
about the crafted run list, and the host functions block_frame / paf_lines of panagram_amd/synteny.py.  The GPU tests hold
k_run_blocks to the model; this file holds the model to the definitions."""
import numpy as np
import pytest

from panagram_amd import synteny
from tests import blocks_ref as br
from tests import synteny_ref as sr

K = sr.PLANTED_K
NO = sr.NO_MATE
WIDE = dict(min_run=1, max_gap=1000, max_shift=100)


def _case(name, k=K):
    case = br.planted_cases(k)[name]
    keys, _, _, _ = sr.side_kmers([sr.ascii_of(c) for c in case[0]], k)
    assert len(np.unique(keys)) == len(keys)  # the premise: every k-mer of A is distinct, both strands counted
    return br.case_runs(case, k)


def _as_runs(blks):
    return np.asarray(blks)[:, :4].tolist()


def test_with_unit_gap_the_blocks_are_the_runs():
    # the crafted mates of the runs' own suite, in kind: stretches on both strands, the three breaks, contigs of 0 and 1 positions
    m = np.array([10, 12, 16, 14, 15, 13, 11, NO, 21, 23, 20, NO, 4, 6, 7, NO - 1], np.uint32)
    nk = [11, 0, 3, 1, 0, 1]
    runs = sr.runs(m, nk)
    for max_shift in (0, 100):
        blks = br.blocks(runs, [1 << 31], 1, 1, max_shift)
        assert _as_runs(blks) == runs.tolist()
        assert (blks[:, 5] == runs[:, 2] - runs[:, 1]).all() and (blks[:, 6] == 1).all() and (blks[:, 7] == 0).all()
        assert blks[:, 4].tolist() == [br.last_mate(int(r[3]), int(r[2] - r[1])) for r in runs]
    # diverged random genomes: a run per stretch between substitutions
    rng = np.random.default_rng(3)
    a = [sr.random_codes(3000, 31), sr.random_codes(2000, 32)]
    b = [sr.plant_snps(c, np.flatnonzero(rng.random(len(c)) < 0.02)) for c in a]
    runs, _ = sr.segments([sr.ascii_of(c) for c in a], [sr.ascii_of(c) for c in b[::-1]], K)
    assert len(runs) > 50
    assert _as_runs(br.blocks(runs, [2000, 3000], 1, 1, 0)) == runs.tolist()


def test_substitutions_are_bridged_into_one_block_per_contig():
    runs, mated, lens_b = _case("snps")
    blks = br.blocks(runs, lens_b, **WIDE)
    nk = [900 - K + 1, 700 - K + 1]
    assert blks.tolist() == [[0, 0, nk[0], 0, (nk[0] - 1) << 1, nk[0] - 3 * K, 4, 0],
                             [1, 0, nk[1], 900 << 1, (900 + nk[1] - 1) << 1, nk[1] - 2 * K, 3, 0]]
    assert blks[:, 5].sum() == mated
    # every link of a substitution is dA = dB = k + 1: at the bound, and one below it
    assert len(br.blocks(runs, lens_b, 1, K + 1, 0)) == 2
    assert _as_runs(br.blocks(runs, lens_b, 1, K, 0)) == runs.tolist()


def test_insertion_and_deletion_are_shifted_links():
    runs, _, lens_b = _case("indel")
    a0, a1, a2 = br.INS_AT - K + 1, br.DEL_AT - K + 1, 900 - K + 1
    assert runs.tolist() == [[0, 0, a0, 0], [0, br.INS_AT, a1, (br.INS_AT + br.INS_LEN) << 1],
                             [0, br.DEL_AT + br.DEL_LEN, a2, (br.DEL_AT + br.INS_LEN) << 1]]
    kmers = [a0, a1 - br.INS_AT, a2 - br.DEL_AT - br.DEL_LEN]
    last = (a2 - 1 + br.INS_LEN - br.DEL_LEN) << 1
    # both bridged from max_shift = the longer one on
    for shift in (br.INS_LEN, 100):
        assert br.blocks(runs, lens_b, 1, 1000, shift).tolist() == [[0, 0, a2, 0, last, sum(kmers), 3, 2]]
    # the insertion (7 bases) breaks the block below 7, the deletion (5 bases) below 5
    for shift in (br.INS_LEN - 1, br.DEL_LEN):
        blks = br.blocks(runs, lens_b, 1, 1000, shift)
        assert blks[:, [1, 2, 5, 6, 7]].tolist() == [[0, a0, kmers[0], 1, 0], [br.INS_AT, a2, kmers[1] + kmers[2], 2, 1]]
    assert _as_runs(br.blocks(runs, lens_b, 1, 1000, br.DEL_LEN - 1)) == runs.tolist()
    # the gaps: dA = k, dB = k + 7 at the insertion; dA = k + 5, dB = k at the deletion
    assert len(br.blocks(runs, lens_b, 1, K + br.INS_LEN, 100)) == 1
    assert len(br.blocks(runs, lens_b, 1, K + br.INS_LEN - 1, 100)) == 2
    assert len(br.blocks(runs, lens_b, 1, K + br.DEL_LEN - 1, 100)) == 3


def test_inversion_gives_three_blocks_the_middle_one_on_minus():
    runs, _, lens_b = _case("inversion")
    blks = br.blocks(runs, lens_b, **WIDE)
    nx, ny = 900 - K + 1, 700 - K + 1
    assert blks.tolist() == [[0, 0, nx, 0, (nx - 1) << 1, nx, 1, 0],
                             [1, 0, 100 - K + 1, 900 << 1, (900 + 100 - K) << 1, 100 - K + 1, 1, 0],
                             [1, 100, 140 - K + 1, ((900 + 140 - K) << 1) | 1, ((900 + 100) << 1) | 1, 40 - K + 1, 1, 0],
                             [1, 140, ny, (900 + 140) << 1, (900 + ny - 1) << 1, ny - 140, 1, 0]]


def test_translocated_block_lies_on_the_other_chromosome():
    runs, _, lens_b = _case("translocation")
    assert lens_b == [600, 1000]
    blks = br.blocks(runs, lens_b, **WIDE)
    rows = br.block_rows(blks, K, ["x", "y"], lens_b, ["bx", "by"])
    # x: its head on bx, the moved block on by, its tail on bx again — the tail's predecessor is the moved block: three blocks
    assert rows[:3] == [("x", 0, 200, "bx", 0, 200, "+", 200 - K + 1, 1, 0), ("x", 200, 500, "by", 300, 600, "+", 300 - K + 1, 1, 0),
                        ("x", 500, 900, "bx", 200, 600, "+", 400 - K + 1, 1, 0)]
    # y: up to the inversion, the inversion, up to the insertion point, and behind the moved block, 300 bases further on in B
    assert [r[:7] for r in rows[3:]] == [("y", 0, 100, "by", 0, 100, "+"), ("y", 100, 140, "by", 100, 140, "-"),
                                         ("y", 140, 300, "by", 140, 300, "+"), ("y", 300, 700, "by", 600, 1000, "+")]
    # a gap and a shift wide enough bridge the moved block's place in y: dA = k, dB = k + 300
    merged = br.blocks(runs, lens_b, 1, 1000, 300)
    assert merged[-1].tolist()[:3] == [1, 140, 700 - K + 1] and merged[-1].tolist()[5:] == [160 - K + 1 + 400 - K + 1, 2, 1]


def test_stray_run_breaks_a_block_unless_dropped():
    runs, _, lens_b = _case("stray")
    n = br.STRAY_KMERS
    q0 = 400 + K + n - 1
    assert runs.tolist() == [[0, 0, 400 - K + 1, 0], [0, 400, 400 + n, (lens_b[0] + 200) << 1], [0, q0, lens_b[0] - K + 1, q0 << 1]]
    assert _as_runs(br.blocks(runs, lens_b, 1, 1000, 100)) == runs.tolist()
    assert _as_runs(br.blocks(runs, lens_b, n, 1000, 100)) == runs.tolist()
    one = br.blocks(runs, lens_b, n + 1, 1000, 100)
    # (positions 400 - K + 1 .. q0 - 1 of A lie in neither run: 2 K + n - 2 of them)
    assert one.tolist() == [[0, 0, lens_b[0] - K + 1, 0, (lens_b[0] - K) << 1, lens_b[0] - K + 1 - (2 * K + n - 2), 2, 0]]


def test_blocks_do_not_cross_a_contig_edge_of_b():
    runs, _, lens_b = _case("three_b")
    # the three runs lie k positions apart on both genomes: everything holds but the contig of B
    assert runs.tolist() == [[0, 0, 300 - K + 1, 0], [0, 300, 600 - K + 1, 600], [0, 600, 900 - K + 1, 1200]]
    assert _as_runs(br.blocks(runs, lens_b, **WIDE)) == runs.tolist()
    assert len(br.blocks(runs, [900], **WIDE)) == 1
    assert len(br.blocks(runs, [300, 0, 600], **WIDE)) == 2  # (an empty contig of B holds no position)


def test_crafted_runs_hold_what_they_promise():
    runs, ncontigs, lens_b, params, want = br.crafted_runs()
    assert ncontigs == 14 and len(lens_b) == 3 and sum(lens_b) == 1 << 31
    per = np.bincount(runs[:, 0], minlength=ncontigs).tolist()
    assert per == [3 * br.CHUNK + 77, br.CHUNK + 1, br.CHUNK, 2 * br.CHUNK + 10, 0, 1, 1, 0, 3, 2, 7, 13, 9, 4]
    blks = br.blocks(runs, lens_b, **params)
    assert blks[:, [0, 1, 2, 3, 4, 6, 7]].tolist() == br.want_blocks(runs, want).tolist()
    n = runs[:, 2] - runs[:, 1]
    # contig 0: the block over three chunks, whose sums need the chunks before; dropped runs at the edges of a tile and of a chunk
    c0 = runs[runs[:, 0] == 0]
    big = blks[(blks[:, 0] == 0)][1]
    assert big[6] > 2 * br.CHUNK and big[5] == 4 * big[6] and big[7] == 82
    assert (c0[:, 2] - c0[:, 1])[[512, 767, 2 * br.CHUNK - 1, 2 * br.CHUNK]].tolist() == [1, 1, 1, 1]
    assert ((c0[:, 2] - c0[:, 1])[[63, 64, 255, 256, br.CHUNK - 1, br.CHUNK]] == 4).all()
    # contig 1 on strand - throughout; contig 3's middle chunk all dropped
    assert (runs[runs[:, 0] == 1][:, 3] & 1).all()
    c3 = runs[runs[:, 0] == 3]
    assert ((c3[:, 2] - c3[:, 1])[br.CHUNK:2 * br.CHUNK] < params["min_run"]).all()
    assert br.link(tuple(c3[br.CHUNK - 1]), tuple(c3[2 * br.CHUNK]), lens_b, params["max_gap"], params["max_shift"]) == (True, True)
    # contigs 8 and 9 go on as one block would: as ONE contig they link
    c8, c9 = runs[runs[:, 0] == 8], runs[runs[:, 0] == 9]
    assert br.link(tuple(c8[-1]), (8, *c9[0][1:]), lens_b, params["max_gap"], params["max_shift"]) == (True, False)
    # contig 10: the pair across B's contig edge links once the edge is gone
    c10 = runs[runs[:, 0] == 10]
    assert br.link(tuple(c10[5]), tuple(c10[6]), [sum(lens_b)], params["max_gap"], params["max_shift"]) == (True, False)
    assert br.link(tuple(c10[5]), tuple(c10[6]), lens_b, params["max_gap"], params["max_shift"]) == (False, False)
    assert br.link(tuple(c10[2]), tuple(c10[3]), [sum(lens_b)], 1, 0) == (True, False)
    # contigs 11 and 12: every condition of the link refuses some pair BY ITSELF, on either strand where it has one — a rule
    # that left a condition out, or tested one twice, gives other blocks
    G, S = params["max_gap"], params["max_shift"]
    alone = {}
    for c in (10, 11, 12):
        mine = [tuple(r) for r in runs[runs[:, 0] == c].tolist()]
        for i, j in zip(mine, mine[1:]):
            failed = br.failed_conditions(i, j, lens_b, G, S)
            assert (not failed) == br.link(i, j, lens_b, G, S)[0]
            if len(failed) == 1:
                alone.setdefault(failed[0], set()).add(j[3] & 1)
    assert alone == {"strand": {0, 1}, "dA <= max_gap": {0, 1}, "dB >= 1": {0, 1}, "dB <= max_gap": {0, 1}, "shift": {0, 1},
                     "contig of B": {0}}
    c11, c12 = ([tuple(r) for r in runs[runs[:, 0] == c].tolist()] for c in (11, 12))
    for mine, past_a, past_b in ((c11, 2, 4), (c12, 7, 2)):
        # one past dA's bound / dB's bound: refused at max_gap, linked at max_gap + 1, and the pair before it is AT the bound
        for j in (past_a, past_b):
            assert br.link(mine[j - 1], mine[j], lens_b, G, S) == (False, False)
            assert br.link(mine[j - 1], mine[j], lens_b, G + 1, S) == (True, True)
        assert br.failed_conditions(mine[past_a - 1], mine[past_a], lens_b, G, S) == ["dA <= max_gap"]
        assert br.failed_conditions(mine[past_b - 1], mine[past_b], lens_b, G, S) == ["dB <= max_gap"]
    for i, j in ((c11[0], c11[1]), (c11[2], c11[3]), (c12[0], c12[1])):  # at a gap's bound and at the shift's at once
        assert br.link(i, j, lens_b, G, S) == (True, True)
        assert br.link(i, j, lens_b, G - 1, S) == (False, False) and br.link(i, j, lens_b, G, S - 1) == (False, False)
    # contig 13: the largest words
    assert blks[blks[:, 0] == 13][:, [3, 4]].tolist() == [[((1 << 31) - 15) << 1, NO - 1], [NO - 2, ((1 << 31) - 2 - 3 - 9 - 3) << 1 | 1]]
    assert (n >= 1).all() and runs[:, 3].max() == NO - 2


# ---------------------------------------------------------------------------
# panagram_amd/synteny.py
# ---------------------------------------------------------------------------
def test_block_frame_and_paf_lines_by_hand():
    k = 5
    lens_b = [100, 0, 50]
    #         contig start end  mate_first      mate_last       kmers runs shifted
    blks = [(0, 2, 40, 10 << 1, 51 << 1, 30, 3, 1),                   # +: B [10, 51 + 5); an insertion in B: 46 bases against 42
            (1, 0, 20, (130 << 1) | 1, (108 << 1) | 1, 18, 2, 1),     # -: B global [108, 135) = contig 2, [8, 35)
            (1, 30, 33, 0, 2 << 1, 3, 1, 0)]
    cols = [np.array(c, np.uint32) for c in zip(*blks)]
    f = synteny.block_frame(*cols, k, ["a0", "a1"], lens_b, ["b0", "b1", "b2"])
    assert list(f.columns) == ["chrA", "startA", "endA", "chrB", "startB", "endB", "strand", "kmers", "runs", "shifted"]
    assert f.values.tolist() == [["a0", 2, 44, "b0", 10, 56, "+", 30, 3, 1], ["a1", 0, 24, "b2", 8, 35, "-", 18, 2, 1],
                                 ["a1", 30, 37, "b0", 0, 7, "+", 3, 1, 0]]
    assert [tuple(r) for r in f.values.tolist()] == br.block_rows(np.array(blks), k, ["a0", "a1"], lens_b, ["b0", "b1", "b2"])
    assert synteny.block_frame(*cols, k, ["a0", "a1"], lens_b, ["b0", "b1", "b2"], min_len=18)["kmers"].tolist() == [30, 18]
    paf = synteny.paf_lines(f, {"a0": 500, "a1": 60}, {"b0": 100, "b1": 0, "b2": 50})
    assert paf == ["a0\t500\t2\t44\t+\tb0\t100\t10\t56\t30\t46\t255\trn:i:3\tsh:i:1",
                   "a1\t60\t0\t24\t-\tb2\t50\t8\t35\t18\t27\t255\trn:i:2\tsh:i:1",
                   "a1\t60\t30\t37\t+\tb0\t100\t0\t7\t3\t7\t255\trn:i:1\tsh:i:0"]
    # the summary and the chromosome map work on blocks as on segments
    s = synteny.summary_frame(f)
    assert list(s.columns) == ["chrA", "chrB", "strand", "segments", "kmers"] and s.values.tolist()[-1] == ["*", "*", "*", 3, 51]
    assert synteny.chromosome_map(f)[["chrA", "chrB", "kmers"]].values.tolist() == [["a0", "b0", 30], ["a1", "b2", 18]]
    empty = synteny.block_frame(*[np.zeros(0, np.uint32)] * 8, k, ["a0"], lens_b, ["b0", "b1", "b2"])
    assert len(empty) == 0 and list(empty.columns) == list(f.columns) and synteny.paf_lines(empty, {}, {}) == []


def test_block_frame_refuses_blocks_outside_b():
    k = 5
    one = lambda *b: [np.array([v], np.uint32) for v in b]
    with pytest.raises(ValueError, match="across a contig edge"):
        synteny.block_frame(*one(0, 0, 10, 90 << 1, 99 << 1, 10, 1, 0), k, ["a"], [100, 50], ["b0", "b1"])
    with pytest.raises(ValueError, match="outside genome B"):
        synteny.block_frame(*one(0, 0, 10, 140 << 1, 149 << 1, 10, 1, 0), k, ["a"], [100, 50], ["b0", "b1"])
    with pytest.raises(ValueError, match="outside genome B"):  # positions of B that descend on +
        synteny.block_frame(*one(0, 0, 10, 40 << 1, 30 << 1, 10, 1, 0), k, ["a"], [100, 50], ["b0", "b1"])
    with pytest.raises(ValueError, match="two strands"):
        synteny.block_frame(*one(0, 0, 10, 40 << 1, (49 << 1) | 1, 10, 1, 0), k, ["a"], [100, 50], ["b0", "b1"])
    with pytest.raises(ValueError, match="min_len"):
        synteny.block_frame(*one(0, 0, 10, 40 << 1, 49 << 1, 10, 1, 0), k, ["a"], [100, 50], ["b0", "b1"], min_len=0)
    with pytest.raises(ValueError, match="differ in length"):
        synteny.block_frame(*(one(0, 0, 10, 40 << 1, 49 << 1, 10, 1)[:7] + [np.zeros(2, np.uint32)]), k, ["a"], [100, 50], ["b0", "b1"])
