"""CPU: the numpy model of the variants (tests/variants_ref.py) on planted genomes whose differences follow by construction, the
invariant that ties the records to the blocks, the crafted run list's promises counted, and the host side of `synteny --variants`:
synteny.variant_frame, vcf_lines, apply_variants, and the sub-command's argument errors."""
import numpy as np
import pytest

from panagram_amd import synteny
from tests import blocks_ref as br
from tests import synteny_ref as sr
from tests import variants_ref as vr

K = sr.PLANTED_K


@pytest.fixture(scope="module")
def cases():
    return vr.planted_cases(K)


@pytest.fixture(scope="module")
def crafted():
    runs, a, b, k, params, marks = vr.crafted()
    return runs, a, b, k, params, marks, vr.variants(runs, a, b, k, **params)


def _model(case):
    a, b, params, want = case
    runs, _ = vr.case_runs(case, K)
    return runs, vr.variants(runs, a, b, K, **params)


def test_all_kmers_of_the_planted_genomes_are_distinct(cases):
    for name, (a, _, _, want) in cases.items():
        if name in ("n_and_dup", "tandem"):
            continue  # (a k-mer held twice on purpose / a repeat shorter than k: distinct all the same, checked below)
        keys = sr.side_kmers(a, K)[0]
        assert len(np.unique(keys)) == len(keys), name
    keys = sr.side_kmers(cases["tandem"][0], K)[0]
    assert len(np.unique(keys)) == len(keys)
    keys = sr.side_kmers(cases["n_and_dup"][0], K)[0]
    assert len(keys) - len(np.unique(keys)) == 1


@pytest.mark.parametrize("name", ["snps", "indel", "stray", "inverted", "tandem", "near", "long", "n_and_dup", "b_start", "a_end"])
def test_model_returns_the_planted_differences(cases, name):
    a, b, params, want = cases[name]
    _, m = _model(cases[name])
    got = [(int(r[0]), int(r[1]), int(r[5] >> 1) & 7, al[0], al[1], int(r[5]) & 1) for r, al in zip(m["records"], m["alleles"])]
    assert got == [(c, q, cls, vr.norm(a[c])[q:q + n], alt, strand) for c, q, cls, n, alt, strand in want]
    assert m["links"] == sum(m["classes"]) and sum(m["classes"][1:]) == len(want)


def test_planted_differences_in_detail(cases):
    # the insertion and the deletion of tests/blocks_ref.py: dA = 15, dB = 22 at posA 300; dA = 20, dB = 15 at posA 600
    runs, m = _model(cases["indel"])
    assert [(r[1], r[2], r[4], (r[5] >> 1) & 7) for r in m["records"].tolist()] == [(300, 0, 7, vr.INS), (600, 5, 0, vr.DEL)]
    d = [(runs[i + 1][1] - (runs[i][2] - 1), (runs[i + 1][3] >> 1) - ((runs[i][3] >> 1) + runs[i][2] - runs[i][1] - 1)) for i in (0, 1)]
    assert d == [(15, 22), (20, 15)]
    # the stray run dropped: one 19-base mnp between two bridged stretches
    _, m = _model(cases["stray"])
    assert m["records"][:, [1, 2, 4]].tolist() == [[400, 19, 19]] and m["classes"] == [0, 0, 1, 0, 0, 0] and len(m["blocks"]) == 1
    assert m["records"][0, 6] == sum(x != y for x, y in zip(*m["alleles"][0]))
    # ... and kept, it breaks the block: no link, no variant
    a, b, _, _ = cases["stray"]
    assert vr.variants(vr.case_runs(cases["stray"], K)[0], a, b, K, min_run=1, max_gap=1000, max_shift=100)["links"] == 0
    # the inversion's variants lie on strand 1, the flanks' blocks have none
    _, m = _model(cases["inverted"])
    assert [r[5] & 1 for r in m["records"].tolist()] == [1, 1, 1] and [len(blk[5]) for blk in m["blocks"]] == [0, 3, 0]
    # the tandem repeat: the flanks overlap by two units, the difference stands at the repeat's first unit
    runs, m = _model(cases["tandem"])
    assert [(r[1], r[2], r[4]) for r in m["records"].tolist()] == [(300, 4, 0), (612, 0, 4)]
    assert runs[1][1] - (runs[0][2] - 1) == K - 4 and runs[2][1] - (runs[1][2] - 1) == K - 8   # dA below k: t = 8 both times
    # alleles beyond 32 bases; the mnp's every base differs
    _, m = _model(cases["long"])
    assert m["records"][:, [2, 4, 6]].tolist() == [[0, 40, 0], [70, 70, 70]]
    # N flags, and the two `same` links of the k-mer held twice (one in either contig that holds it)
    _, m = _model(cases["n_and_dup"])
    assert [r[5] >> 6 for r in m["records"].tolist()] == [1, 1, 1] and m["records"][:, 6].tolist() == [1, 1, 2] and m["classes"][0] == 2
    # the start of B's first contig: strand 1, the last allele inside its first 32 bases
    _, m = _model(cases["b_start"])
    last = m["records"][-1].tolist()
    assert last[5] & 1 == 1 and last[3] + last[4] <= 32 and last[3] >= 1
    # the end of a contig: strand 0, within 32 bases of the end of both sides' last contig
    a, b, _, _ = cases["a_end"]
    _, m = _model(cases["a_end"])
    last = m["records"][-1].tolist()
    assert last[0] == 1 and len(a[1]) - last[1] <= 32 and sum(len(c) for c in b) - last[3] <= 32


def test_the_invariant_holds_on_every_planted_case(cases):
    for name, case in cases.items():
        _, m = _model(case)
        assert m["blocks"] and vr.invariant_holds(m, case[0], case[1], K), name
        # the blocks are those of tests/blocks_ref.py
        blks = br.blocks(vr.case_runs(case, K)[0], [len(c) for c in case[1]], **case[2])
        assert [blk[:5] for blk in m["blocks"]] == blks[:, :5].tolist(), name
        assert m["links"] == int((blks[:, 6] - 1).sum()), name


def test_the_invariant_fails_for_a_wrong_record(cases):
    case = cases["indel"]
    _, m = _model(case)
    m["alleles"][0] = (m["alleles"][0][0], m["alleles"][0][1][:-1] + b"A" if m["alleles"][0][1][-1:] != b"A" else m["alleles"][0][1][:-1] + b"C")
    assert not vr.invariant_holds(m, case[0], case[1], K)


def test_crafted_list_holds_what_it_promises(crafted):
    runs, a, b, k, params, marks, m = crafted
    lens_b = [len(c) for c in b]
    offs = np.concatenate([[0], np.cumsum(lens_b)])
    G, S, R = params["max_gap"], params["max_shift"], params["min_run"]
    assert len(runs) > 3 * vr.CHUNK + 77 and 900_000 < sum(map(len, a)) + sum(lens_b) < 1_300_000
    rec = m["records"]
    strand, cls, la, lb = rec[:, 5] & 1, (rec[:, 5] >> 1) & 7, rec[:, 2], rec[:, 4]
    # links of every class on both strands
    assert m["classes"][0] > 1000
    for c in range(1, 6):
        for s in (0, 1):
            assert int(((cls == c) & (strand == s)).sum()) > 100, (c, s)
    # alleles of up to 32 bases that straddle a 32-base word edge, on A's planes and on B's, and on B's on strand 1
    cb = np.searchsorted(offs, rec[:, 3], side="right") - 1
    lo = rec[:, 3] - offs[cb]
    for pos, n in ((rec[:, 1], la), (lo, lb)):
        assert int(((n >= 2) & (n <= 32) & (pos % 32 + n > 32)).sum()) > 100
    assert int(((lb >= 2) & (lb <= 32) & (lo % 32 + lb > 32) & (strand == 1)).sum()) > 50
    # alleles beyond 32 bases and beyond a thousand, flanks that overlap around an indel (lenA == 0 or lenB == 0 with dA or dB below k)
    assert int((la > 32).sum()) > 1000 and int((la > 4000).sum()) >= 4 and int((lb > 4000).sum()) >= 4
    assert int((((cls == vr.INS) & (lb == 4)) | ((cls == vr.DEL) & (la == 4))).sum()) > 500
    # N flags, on records of either strand
    assert int(((rec[:, 5] >> 6) & (strand == 0)).sum()) > 5 and int(((rec[:, 5] >> 6) & (strand == 1)).sum()) > 2
    # strand 1 at the start of B's first contig: the window would begin before base 0
    assert int(((strand == 1) & (cb == 0) & (lb > 0) & (lo + lb < 32)).sum()) >= 1
    last1 = runs[marks["first_row"][2] - 1]
    assert (last1[3] >> 1) - (last1[2] - last1[1] - 1) == 0 and last1[2] + k - 1 == len(a[1])  # contig 1 ends on B's base 0 and A's last
    # the predecessor in the last lane of the wave / the tile / the chunk before
    kept = (runs[:, 2] - runs[:, 1]) >= R
    for name in ("wave", "tile", "chunk"):
        j = marks[name]
        assert j - marks["first_row"][0] in (vr.WAVE, vr.TILE, vr.CHUNK) and kept[j] and kept[j - 1]
        assert br.link(tuple(runs[j - 1]), tuple(runs[j]), lens_b, G, S)[0], name
    # ... and of a chunk two chunks back, with only dropped runs between
    j = marks["two_chunks"]
    first = marks["first_row"][2]
    assert j - first == 2 * vr.CHUNK and kept[j] and kept[j - vr.CHUNK - 1] and not kept[j - vr.CHUNK:j].any()
    assert br.link(tuple(runs[j - vr.CHUNK - 1]), tuple(runs[j]), lens_b, G, S)[0]
    hit = rec[(rec[:, 0] == 2) & (rec[:, 1] + rec[:, 2] == runs[j][1])]
    assert len(hit) == 1 and hit[0, 2] == hit[0, 4] == vr.CHUNK + 3 and hit[0, 6] > 0
    # dropped runs in the first and the last lane of a tile and on both sides of a chunk edge
    r0 = marks["first_row"][0]
    assert not kept[[r0 + 512, r0 + 767, r0 + 2 * vr.CHUNK - 1, r0 + 2 * vr.CHUNK]].any()
    # pairs at each bound and one past each, on both strands: what refuses a pair is that bound alone
    want = [[], ["dA <= max_gap"], [], ["dB <= max_gap"], [], ["shift"], [], ["shift"], []]
    for r in marks["bounds"]:
        got = [br.failed_conditions(tuple(runs[r + i]), tuple(runs[r + i + 1]), lens_b, G, S) for i in range(len(want))]
        assert got == want, (r, got)
    assert (runs[marks["bounds"][0]][3] & 1, runs[marks["bounds"][1]][3] & 1) == (0, 1)
    # (no invariant here: the runs are laid by hand over sequences that do not match along them)


# ---------------------------------------------------------------------------
# the host side of `synteny --variants`
# ---------------------------------------------------------------------------
class _Seqs:
    """what variant_frame asks of a sequence set: unpack(contig), counted"""

    def __init__(self, contigs):
        self.contigs, self.calls = [vr.norm(c) for c in contigs], []

    def unpack(self, i):
        self.calls.append(i)
        return self.contigs[i]


def _frame(case, with_seqs=True):
    a, b, params, _ = case
    runs, _ = vr.case_runs(case, K)
    m = vr.variants(runs, a, b, K, **params)
    sa, sb = _Seqs(a), _Seqs(b)
    names_a, names_b = [f"a{i}" for i in range(len(a))], [f"b{i}" for i in range(len(b))]
    f = synteny.variant_frame(*m["records"].T, m["words"][:, 0], m["words"][:, 1], names_a, [len(c) for c in b], names_b,
                              sa if with_seqs else None, sb if with_seqs else None)
    return f, m, sa, sb


def test_variant_frame_by_hand(cases):
    f, m, sa, sb = _frame(cases["indel"], with_seqs=False)     # short alleles without N: the words suffice
    a, b = cases["indel"][:2]
    assert list(f.columns) == synteny.VARIANT_COLUMNS
    assert f.values.tolist() == [["a0", 300, 0, "b0", 300, 7, "+", "ins", 0, "", b[0][300:307].decode()],
                                 ["a0", 600, 5, "b0", 607, 0, "+", "del", 0, a[0][600:605].decode(), ""]]
    assert f.attrs["anchor"] == [chr(a[0][299]), chr(a[0][599])]
    # strand -: posB is the lowest base of B's range, alt in A's orientation
    f, m, sa, sb = _frame(cases["inverted"])
    a, b = cases["inverted"][:2]
    assert f["strand"].tolist() == ["-"] * 3 and f["class"].tolist() == ["snp", "ins", "del"] and not sa.calls and not sb.calls
    snp = f.iloc[0]
    assert vr.revcomp(b[0][snp.posB:snp.posB + 1]).decode() == snp.alt != snp.ref == chr(a[0][360])
    ins = f.iloc[1]
    assert vr.revcomp(b[0][ins.posB:ins.posB + 5]).decode() == ins.alt and ins.posA == 430
    # alleles beyond 32 bases come off the sequence sets, each contig unpacked once and only then
    f, m, sa, sb = _frame(cases["long"])
    a, b = cases["long"][:2]
    assert f["alt"].tolist() == [b[0][300:340].decode(), b[0][740:810].decode()] and f["ref"].tolist() == ["", a[0][700:770].decode()]
    assert sa.calls == [0] and sb.calls == [0]
    with pytest.raises(ValueError):
        _frame(cases["long"], with_seqs=False)
    # N-flagged alleles show N at those bases
    f, m, sa, sb = _frame(cases["n_and_dup"])
    assert f[["posA", "ref", "alt"]].values.tolist()[::2] == [[300, chr(cases["n_and_dup"][0][0][300]), "N"],
                                                              [798, vr.norm(cases["n_and_dup"][0][0])[798:801].decode(),
                                                               vr.norm(cases["n_and_dup"][1][0])[798:801].decode()]]
    assert f.iloc[1][["ref", "alt"]].tolist() == ["N", "C"] and f.iloc[2]["alt"][2] == "N"
    # the second side's contig and offset: a variant in B's second contig
    f, m, _, _ = _frame(cases["a_end"])
    assert f["chrA"].tolist() == ["a1", "a1"] and f["chrB"].tolist() == ["b1", "b1"] and f["posB"].tolist() == [280, 318]
    # refused: arrays of different lengths, a class outside 1..5, a variant outside B
    rec, words = m["records"], m["words"]
    with pytest.raises(ValueError):
        synteny.variant_frame(*rec.T[:6], rec[:1, 6], words[:, 0], words[:, 1], ["a0", "a1"], [300, 336], ["b0", "b1"])
    bad = rec.copy()
    bad[0, 5] &= ~0xE
    with pytest.raises(ValueError):
        synteny.variant_frame(*bad.T, words[:, 0], words[:, 1], ["a0", "a1"], [300, 336], ["b0", "b1"])
    with pytest.raises(ValueError):
        synteny.variant_frame(*rec.T, words[:, 0], words[:, 1], ["a0", "a1"], [300, 30], ["b0", "b1"])
    empty = synteny.variant_frame(*[[]] * 9, ["a"], [10], ["b"])
    assert list(empty.columns) == synteny.VARIANT_COLUMNS and len(empty) == 0


def test_vcf_lines_by_hand(cases):
    f, m, _, _ = _frame(cases["indel"])
    a, b = cases["indel"][:2]
    lines = synteny.vcf_lines(f, {"a0": len(a[0])}, "genomeB")
    head = [ln for ln in lines if ln.startswith("#")]
    assert head[0] == "##fileformat=VCFv4.2" and head[1] == f"##contig=<ID=a0,length={len(a[0])}>"
    assert head[-1] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tgenomeB"
    assert sum(ln.startswith("##INFO=<ID=") for ln in head) == 5 and any(ln.startswith("##FILTER=<ID=N,") for ln in head)
    anchor_i, anchor_d = chr(a[0][299]), chr(a[0][599])
    assert lines[len(head):] == [
        f"a0\t300\t.\t{anchor_i}\t{anchor_i}{b[0][300:307].decode()}\t.\tPASS\tCLASS=ins;BCHR=b0;BPOS=301;STRAND=+;MISM=0\tGT\t1",
        f"a0\t600\t.\t{anchor_d}{a[0][600:605].decode()}\t{anchor_d}\t.\tPASS\tCLASS=del;BCHR=b0;BPOS=608;STRAND=+;MISM=0\tGT\t1"]
    # a snp stands at its own base, 1-based, without an anchor; an N-flagged record is filtered N
    f, m, _, _ = _frame(cases["n_and_dup"])
    a, b = cases["n_and_dup"][:2]
    body = [ln.split("\t") for ln in synteny.vcf_lines(f, {"a0": 1000, "a1": len(a[1])}, "B") if not ln.startswith("#")]
    assert [ln[:7] for ln in body[:2]] == [["a0", "301", ".", chr(a[0][300]), "N", ".", "N"], ["a0", "601", ".", "N", "C", ".", "N"]]
    # long alleles whole, and a complex variant behind its anchor
    f, m, _, _ = _frame(cases["long"])
    a, b = cases["long"][:2]
    body = [ln.split("\t") for ln in synteny.vcf_lines(f, {"a0": 1200}, "B") if not ln.startswith("#")]
    assert body[0][1:5] == ["300", ".", chr(a[0][299]), chr(a[0][299]) + b[0][300:340].decode()]
    assert body[1][1:5] == ["701", ".", a[0][700:770].decode(), b[0][740:810].decode()] and body[1][7].endswith("MISM=70")
    f, m, _, _ = _frame(cases["near"])
    a, b = cases["near"][:2]
    body = [ln.split("\t") for ln in synteny.vcf_lines(f, {"a0": 900}, "B") if not ln.startswith("#")]
    assert body[1][1:5] == ["500", ".", a[0][499:501].decode(), b[0][499:505].decode()] and "CLASS=complex" in body[1][7]
    # every line has ten fields, positions ascend inside a chromosome
    for ln in body:
        assert len(ln) == 10 and ln[8:] == ["GT", "1"]
    with pytest.raises(ValueError):  # (a frame of another making: no anchor bases)
        synteny.vcf_lines(f.__class__(f.values, columns=f.columns), {"a0": 900}, "B")


def test_apply_variants_performs_the_invariants_substitution(cases):
    for name, case in cases.items():
        f, m, _, _ = _frame(case)
        a, b = case[:2]
        for blk in m["blocks"]:
            c, s, e = blk[:3]
            got = synteny.apply_variants(vr.norm(a[c]), f, s, e + K - 1, chrom=f"a{c}")
            assert got == vr.block_b_range(blk, b, K), (name, blk[:3])
    # by hand: a deletion, an insertion and a substitution
    import pandas as pd
    f = pd.DataFrame([["c", 2, 2, "x", 0, 0, "+", "del", 0, "GT", ""], ["c", 6, 0, "x", 0, 2, "+", "ins", 0, "", "TT"],
                      ["c", 8, 1, "x", 0, 1, "+", "snp", 1, "A", "C"], ["d", 0, 1, "x", 0, 1, "+", "snp", 1, "A", "G"]],
                     columns=synteny.VARIANT_COLUMNS)
    assert synteny.apply_variants(b"ACGTACGTAC", f, chrom="c") == b"ACACTTGTCC"
    assert synteny.apply_variants(b"ACGTACGTAC", f, 4, 8, chrom="c") == b"ACTTGT"      # only the variants inside the range
    with pytest.raises(ValueError):
        synteny.apply_variants(b"ACGTACGTAC", f.iloc[[1, 0]], chrom="c")


def test_variant_summary_by_hand(cases):
    f, m, _, _ = _frame(cases["n_and_dup"])
    s = synteny.variant_summary_frame(f, m["classes"], m["links"])
    assert list(s.columns) == synteny.VARIANT_SUMMARY_COLUMNS
    assert s.values.tolist() == [["snp", 2, 2, 2], ["mnp", 1, 3, 3], ["ins", 0, 0, 0], ["del", 0, 0, 0], ["complex", 0, 0, 0],
                                 ["same", 2, 0, 0], ["links", 5, 5, 5]]
    with pytest.raises(ValueError):
        synteny.variant_summary_frame(f, m["classes"], m["links"] + 1)
    with pytest.raises(ValueError):
        synteny.variant_summary_frame(f.iloc[1:], m["classes"], m["links"])


def test_synteny_variants_argument_errors(capsys):
    """refused before the index is opened"""
    from panagram_amd.__main__ import main
    for flags, text in ((["--blocks", "--variants"], "exclude each other"), (["--vcf"], "--vcf needs --variants"),
                        (["--blocks", "--vcf"], "--vcf needs --variants"), (["--variants", "--paf"], "need --blocks"),
                        (["--paf"], "need --blocks"), (["--max-gap", "10"], "need --blocks"),
                        (["--variants", "--min-len", "5"], "--min-len")):
        with pytest.raises(SystemExit) as ei:
            main(["synteny", "/nonexistent", "g0", "g1"] + flags)
        assert ei.value.code == 2 and text in capsys.readouterr().err, flags
