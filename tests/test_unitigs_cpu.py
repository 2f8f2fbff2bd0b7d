"""CPU: the model of pg_unitigs.hip (tests/unitigs_ref.py) held to a brute force over strings on the crafted samples and on seeded
random graphs, to the partition invariant and to maximality; the crafted sample held to its promises; panagram_amd/novel.py's
unitig frame, FASTA text and statistics on hand-made arrays; the `novel` subcommand's refusal of --min-unitig-bases alone; and
the premise of tests/test_gpu_novel_unitigs_e2e.py under the model."""
import numpy as np
import pytest

from panagram_amd import novel as nov
from tests import novel_ref as NR
from tests import unitigs_ref as UR

KS = UR.KS
THRESHOLDS = [1, 2, 3]


@pytest.mark.parametrize("k", KS)
def test_model_equals_the_brute_force_on_the_crafted_sample(k):
    table, sets, _ = UR.crafted(k)
    for mc in THRESHOLDS:
        nodes, lk, lb, U = UR.crafted_model(k, mc)
        strings = UR.brute_nodes(table, sets, k, mc)
        assert strings == UR.strings_of(nodes, k)
        assert UR.brute_unitigs(strings) == U
        UR.check_partition(U, nodes, k)
        UR.check_maximal(U, nodes, k)
        assert lk.tolist() == sorted(nodes) and len(lb) == len(nodes)


def test_model_equals_the_brute_force_on_random_graphs():
    cycles = palindromes = 0
    for seed in range(200):
        k, nodes = UR.random_graph(seed)
        U = UR.unitigs(nodes, k)
        assert UR.brute_unitigs(UR.strings_of(nodes, k)) == U, seed
        UR.check_partition(U, nodes, k)
        UR.check_maximal(U, nodes, k)
        cycles += sum(c for _, _, _, c in U)
        palindromes += sum(1 for x in nodes if UR.rc(x, k) == x)
    assert cycles >= 10 and palindromes >= 10  # (the graphs hold what the rule's exclusions are about)


def test_link_bytes_by_hand():
    """k = 3, the nodes AAC (= GTT), ACG (= CGT) and CGA (= TCG), worked out on paper:
    AAC  out: ACG (G).  in: none of AAA, CAA, GAA, TAA is a node.
    ACG  out: CGA (A) and CGT (T), which is rc(ACG) — a hairpin.  in: AAC (A) alone.
    CGA  out: none of GAA, GAC, GAG, GAT.  in: ACG (A) and TCG (T), which is rc(CGA).
    AAC -> ACG is compactable (one way out, one way in, two nodes); ACG has two ways out: AACG and CGA are the unitigs."""
    k = 3
    nodes = {UR.canon(int(s.translate(UR._DIGITS), 4), k): d for s, d in (("AAC", 1), ("ACG", 4), ("CGA", 2))}
    aac, acg, cga = (int(s.translate(UR._DIGITS), 4) for s in ("AAC", "ACG", "CGA"))
    assert sorted(nodes) == [aac, acg, cga]  # (all three are spelled canonically)
    assert UR.link_byte(aac, nodes, k) == 0b00000100
    assert UR.link_byte(acg, nodes, k) == 0b00011001
    assert UR.link_byte(cga, nodes, k) == 0b10010000
    assert UR.step(aac, nodes, k) == acg and UR.step(acg, nodes, k) is None
    assert UR.step(UR.rc(acg, k), nodes, k) == UR.rc(aac, k)  # (the same edge from the other strand)
    assert UR.unitigs(nodes, k) == {("AACG", 2, 5, 0), ("CGA", 1, 2, 0)}
    # without AAC the hairpin stands alone: ACG -> CGT is no edge, ACG a unitig of 1
    del nodes[aac]
    assert UR.unitigs(nodes, k) == {("ACG", 1, 4, 0), ("CGA", 1, 2, 0)}


@pytest.mark.parametrize("k", KS)
def test_the_crafted_sample_keeps_its_promises(k):
    table, sets, P = UR.crafted(k)
    nodes, lk, lb, U = UR.crafted_model(k, UR.MIN_COUNT)
    by_seq = {seq: (n, ds, c) for seq, n, ds, c in U}
    assert len(by_seq) == len(U)
    link = dict(zip(lk.tolist(), lb.tolist()))
    assert sum(1 for _, n, _, _ in U if n == 1) >= 2  # (lanes of n = 1 beside the long walk)
    if k < UR.EXACT_FROM_K:  # (2080 canonical 6-mers: chance neighbours everywhere)
        return
    # solid keys in at least three scan blocks of a table at a load of 0.5 at the most
    assert len(nodes) >= 3 * UR.SHORT_CONTIGS and 2 * len(nodes) >= 3 * UR.SCAN_SLOTS
    assert by_seq[P["isolated"]] == (1, 2, 0)
    seq, n = P["insertion"]
    assert by_seq[seq] == (n, 2 * n, 0) and n == UR.INSERTION + k - 1
    assert by_seq[P["long"]] == (UR.LONG_KMERS, 2 * UR.LONG_KMERS, 0)
    bub = P["bubble"]
    # 6 k + 1 bases, the alleles differ at base 3 k: the windows at 0 .. 2 k in front of it, those at 3 k + 1 .. 5 k + 1 behind it
    assert by_seq[bub["left"]][0] == 2 * k + 1 and by_seq[bub["right"]][0] == 2 * k + 1
    assert all(by_seq[arm] == (k, 2 * k, 0) for arm in bub["arms"]) and len(bub["arms"]) == 2
    for x in bub["branch"]:
        assert 2 in (bin(link[x] & 15).count("1"), bin(link[x] >> 4).count("1"))
    tip = P["tip"]
    assert by_seq[tip["tip"]][0] == 5 and by_seq[tip["before"]][0] == k + 1 and by_seq[tip["after"]][0] == 2 * k
    below = P["below"]
    assert all(s in by_seq for s in below["parts"]) and below["whole"] not in by_seq and below["key"] not in nodes
    at1 = {seq: n for seq, n, _, _ in UR.crafted_model(k, UR.MIN_COUNT - 1)[3]}
    assert at1[below["whole"]] == 40 and not set(below["parts"]) & set(at1)
    held = P["held"]
    assert all(s in by_seq for s in held["parts"]) and held["key"] in set(table.tolist()) and held["key"] not in nodes
    assert by_seq[P["homo"]] == (1, 12, 0)
    if k % 2:
        assert by_seq[P["hairpin"]][0] == k + 1  # (the path ends at w: the edge w -> rc(w) is not compactable)
    else:
        assert by_seq[P["palindrome"]][0] == 1
    circ = {n: seq for seq, n, _, c in U if c}
    assert sorted(circ) == [3, 11, UR.CIRCLE]
    for n, keys in ((3, P["sat3"]), (11, P["sat11"])):
        assert int(circ[n][:k].translate(UR._DIGITS), 4) == keys[0] and circ[n][n:] == circ[n][:k - 1]
    z = P["circle"]
    assert circ[UR.CIRCLE][:UR.CIRCLE] in z + z or circ[UR.CIRCLE][:UR.CIRCLE] in UR.revcomp(z) * 2
    assert by_seq[P["entry"]["path"]][0] == k + 5 and by_seq[P["entry"]["cycle"]] [0] == UR.ENTRY_CIRCLE and by_seq[P["entry"]["cycle"]][2] == 0
    assert by_seq[P["deep"]] == (25, 75, 0) and not set(P["once"]) & set(by_seq) and set(P["once"]) <= set(at1)
    at3 = UR.crafted_model(k, 3)[3]
    assert (P["deep"], 25, 75, 0) in at3 and len(at3) < 20 and sum(c for _, _, _, c in at3) == 2


def test_canonical_unitig_and_the_frame():
    assert nov.canonical_unitig("TTGA") == "TCAA" and nov.canonical_unitig("ACGT") == "ACGT" and nov.canonical_unitig("AAC") == "AAC"
    k = 3
    seqs = ["TTGAC", "AACAA", "CCC", "GGTTT", "ACGTT"]           # u: GTCAA -> canonical min(TTGAC, GTCAA) = GTCAA
    circular = [0, 1, 0, 0, 0]
    bases = np.frombuffer("".join(seqs).encode(), np.uint8)
    offsets = np.cumsum([0] + [len(s) for s in seqs[:-1]])
    kmers = np.array([len(s) - k + 1 for s in seqs], np.uint32)
    depth_sum = np.array([7, 9, 5, 3, 2 ** 40], np.uint64)
    f = nov.unitigs_frame(offsets, kmers, depth_sum, circular, bases, k)
    assert list(f.columns) == nov.UNITIG_COLUMNS == ["unitig", "bases", "kmers", "depth", "circular", "sequence"]
    # sorted by (-bases, sequence): the circular one as it came, the linear ones canonicalised
    assert f["sequence"].tolist() == ["AAACC", "AACAA", "AACGT", "GTCAA", "CCC"]
    assert f["unitig"].tolist() == ["u1", "u2", "u3", "u4", "u5"] and f["circular"].tolist() == [0, 1, 0, 0, 0]
    assert f["bases"].tolist() == [5, 5, 5, 5, 3] and f["kmers"].tolist() == [3, 3, 3, 3, 1]
    assert f["depth"].tolist() == [1.0, 3.0, round(2 ** 40 / 3, 2), 2.33, 5.0]
    g = nov.unitigs_frame(offsets, kmers, depth_sum, circular, bases, k, min_unitig_bases=4)
    assert g["sequence"].tolist() == f["sequence"].tolist()[:4] and g["unitig"].tolist() == ["u1", "u2", "u3", "u4"]
    assert len(nov.unitigs_frame([], [], [], [], [], k)) == 0
    with pytest.raises(ValueError, match="min_unitig_bases"):
        nov.unitigs_frame(offsets, kmers, depth_sum, circular, bases, k, min_unitig_bases=-1)


def test_fasta_text_and_statistics(tmp_path):
    k = 21
    rng = np.random.default_rng(3)
    seqs = ["".join("ACGT"[i] for i in rng.integers(0, 4, n)) for n in (200, 80, 81, 21, 50, 50)]
    offsets = np.cumsum([0] + [len(s) for s in seqs[:-1]])
    kmers = [len(s) - k + 1 for s in seqs]
    f = nov.unitigs_frame(offsets, kmers, [3 * n for n in kmers], [0, 0, 1, 0, 0, 0], np.frombuffer("".join(seqs).encode(), np.uint8), k)
    path = tmp_path / "u.fa"
    nov.write_unitigs(f, path)
    text = path.read_text()
    assert text == nov.unitig_fasta(f)
    lines = text.split("\n")
    assert lines[0] == ">u1 bases=200 kmers=180 depth=3.00 circular=0" and [len(x) for x in lines[1:4]] == [80, 80, 40]
    assert lines[4] == ">u2 bases=81 kmers=61 depth=3.00 circular=1" and [len(x) for x in lines[5:7]] == [80, 1]
    assert lines[7].startswith(">u3 bases=80 ") and len(lines[8]) == 80 and lines[9].startswith(">u4 bases=50 ")
    assert max(len(x) for x in lines) == 80 and text.endswith("\n") and text.count(">") == 6
    # it parses back to the frame
    recs = [r.split("\n", 1) for r in text.split(">")[1:]]
    assert [h.split()[0] for h, _ in recs] == f["unitig"].tolist() and [b.replace("\n", "") for _, b in recs] == f["sequence"].tolist()
    st = nov.unitig_stats(f)
    assert list(st) == nov.UNITIG_STAT_NAMES == ["unitigs", "unitig_bases", "unitig_n50", "longest_unitig", "circular_unitigs"]
    # 482 bases: 200 < 241 <= 200 + 81
    assert st == {"unitigs": 6, "unitig_bases": 482, "unitig_n50": 81, "longest_unitig": 200, "circular_unitigs": 1}
    assert nov.unitig_stat_lines(st) == ["unitigs\t6", "unitig_bases\t482", "unitig_n50\t81", "longest_unitig\t200", "circular_unitigs\t1"]
    assert nov.unitig_stats(f[:1])["unitig_n50"] == 200 and nov.unitig_stats(f[1:3])["unitig_n50"] == 81  # (81 of 161: half or more)
    assert nov.unitig_stats(f[:0]) == {"unitigs": 0, "unitig_bases": 0, "unitig_n50": 0, "longest_unitig": 0, "circular_unitigs": 0}


def test_min_unitig_bases_alone_is_refused_before_any_work(tmp_path, capsys):
    from panagram_amd.__main__ import main
    fq = tmp_path / "s.fq"
    fq.write_text("@r\nACGT\n+\nIIII\n")
    for argv, what in ((["novel", str(tmp_path), str(fq), "--min-unitig-bases", "100"], "--min-unitig-bases needs --unitigs"),
                       (["novel", str(tmp_path), str(fq), "--min-unitig-bases", "0"], "--min-unitig-bases needs --unitigs"),
                       (["novel", str(tmp_path), str(fq), "--unitigs", str(tmp_path / "u.fa"), "--min-unitig-bases", "-1"],
                        "--min-unitig-bases not negative")):
        with pytest.raises(SystemExit) as ei:
            main(argv)
        assert ei.value.code == 2
        assert what in capsys.readouterr().err, argv
    assert not (tmp_path / "u.fa").exists()


def test_the_planted_sample_under_the_model():
    """the premise of tests/test_gpu_novel_unitigs_e2e.py: no novel k-mer of the end-to-end FASTA sample repeats, so at min_count 1
    its unitigs are its novel regions' slices; and of the reads at min_count 2 the planted insertion is one unitig"""
    from tests import place_ref as pr
    from tests import screen_ref as SR
    k = pr.E2E["k"]
    keys = SR.e2e_table()[0]
    contigs = NR.e2e_sample()
    _, _, nk, d = NR.novel_counts(keys, [contigs], k)
    assert len(nk) > 3000 and (d == 1).all()
    U = UR.unitigs(UR.nodes_of(nk, d, 1), k)
    rc_, ra, rb, _, _, _, _ = NR.runs(keys, contigs, k)
    slices = {nov.canonical_unitig(contigs[c][a:b + k - 1].decode()) for c, a, b in zip(rc_.tolist(), ra.tolist(), rb.tolist())}
    assert {seq for seq, _, _, _ in U} == slices and not any(c for _, _, _, c in U) and len(slices) == len(rc_) >= 4
    ins = UR.e2e_insertion()
    assert ins in slices
    _, _, nk, d = NR.novel_counts(keys, [pr.joined_reads(NR.e2e_reads()[0])], k)
    assert ins in {seq for seq, _, _, _ in UR.unitigs(UR.nodes_of(nk, d, 2), k)}

