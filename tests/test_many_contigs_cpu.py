"""No GPU: the crafted many-contig sets of tests/many_contigs.py hold what they promise — every length class, the runs of
contigs without a k-mer at the front, in the middle and at the end, N and lower case, the bases within bounds — for every
(contig count, k) that tests/test_gpu_many_contigs.py uses; and the three FASTA readers of the host (search.scan_fasta,
index.read_fasta, and po.fasta_text's own input) agree on the FASTA texts the GPU tests parse, so that what those tests
expect is settled before any GPU run."""
import numpy as np
import pytest

from oracle import pyoracle as po
from panagram_amd import engine, index as pidx, search
from tests import many_contigs as mc

T = engine.tile_positions()
USED = [(n, k) for n in mc.COUNTS for k in (21, 31)] + [(n, 21) for n in mc.REGROWTH if n >= mc.MIN_CRAFTED]


def test_the_tile_is_the_one_the_classes_were_laid_out_for():
    assert T == 1024
    assert [-(-n // 1024) for n in mc.COUNTS] == [2, 3, 3] and mc.MIDDLE > 3  # contigs per thread of k_tile0: a whole share inside the run
    # the regrowth sequence: tile0 needs n + 1 words; room for max(1024, 2 (n + 1)) is made
    cap = 0
    grown = []
    for n in mc.REGROWTH:
        if cap < n + 1:
            grown.append((n + 1, cap))
            cap = max(1024, 2 * (n + 1))
    assert grown == [(11, 0), (1025, 1024), (2052, 2050)]


@pytest.mark.parametrize("ends_empty", [True, False])
@pytest.mark.parametrize("n,k", USED)
def test_crafted_sets_hold_every_class_and_every_run(n, k, ends_empty):
    lens = mc.lengths(k, n, 7, T, ends_empty)
    nk = np.maximum(lens - k + 1, 0)
    assert len(lens) == n
    cl = mc.classes(k, T)
    for name in ("none", "few", "bins", "tiles"):
        for length in cl[name]:
            assert (lens == length).sum() >= 1, (name, length)
    assert sorted(set(nk[np.isin(lens, cl["tiles"])])) == [T - 1, T, T + 1, 2 * T, 2 * T + 1, 4 * T + 1]
    assert sorted(set(nk[np.isin(lens, cl["bins"])])) == [99, 100, 101]
    long_ones = lens[lens >= 5000]
    assert len(long_ones) == len(mc.LONG) and long_ones.max() <= 20006
    # the runs of contigs without a k-mer: front, middle (longer than a thread's share of k_tile0, and holding a whole share), end
    assert (nk[:mc.HEAD] == 0).all()
    m0, mn = mc.middle_run(n)
    per = -(-n // 1024)
    assert mn >= 8 and (nk[m0:m0 + mn] == 0).all()
    shares = [t for t in range(1024) if m0 <= t * per and (t + 1) * per <= m0 + mn]
    assert shares, "no thread of k_tile0 has a share of contigs that sums to 0"
    if ends_empty:
        assert (nk[n - mc.TAIL:] == 0).all()
    else:
        assert nk[n - 1] == 99 and (nk[n - 1 - mc.TAIL:n - 1] == 0).all()
    # equal neighbours in tile0 elsewhere too: single empty contigs between contigs of one tile or less
    assert ((nk[1:-1] == 0) & (nk[:-2] > 0) & (nk[2:] > 0)).sum() > n // 16
    assert mc.MIN_BASES <= lens.sum() <= mc.MAX_BASES, lens.sum()
    # nearly every contig is one tile or less
    assert (nk <= T).mean() > 0.97


def test_the_small_set_of_the_regrowth_sequence():
    lens = mc.lengths(21, 10, 7, T)
    assert len(lens) == 10 and (lens < 21).sum() >= 3 and (lens >= 21).sum() >= 5 and lens[0] == 0


@pytest.mark.parametrize("n,k", [(3000, 21), (1025, 31)])
def test_fragments_are_the_sequence_cut_at_the_lengths(n, k):
    lens = mc.lengths(k, n, 7, T)
    codes = np.random.default_rng(3).integers(0, 4, int(lens.sum()) + 100, dtype=np.uint8)
    contigs = mc.fragments(codes, k, n, 7, T)
    assert [len(c) for c in contigs] == lens.tolist() and mc.total_bases(k, n, 7, T) == lens.sum()
    whole = po.codes_to_ascii(codes[:int(lens.sum())])
    got, want = (np.frombuffer(x, np.uint8) for x in (mc.norm(b"".join(contigs)), whole))
    masked = got == ord("N")
    assert masked.sum() == 47 and np.array_equal(got[~masked], want[~masked])
    kinds = mc.marks(lens, k)
    assert sorted(kinds.values()) == ["lower", "lower", "n", "n", "nrun"]
    for c, what in kinds.items():
        s = contigs[c]
        if what == "lower":
            assert s == s.lower() != s.upper()
        else:
            assert s.count(b"N") == (45 if what == "nrun" else 1)
    nrun = contigs[[c for c, w in kinds.items() if w == "nrun"][0]]
    assert nrun[2 * T - 10:2 * T + 35] == b"N" * 45  # k-mers without a row bit on both sides of the second tile's end
    with pytest.raises(ValueError):
        mc.fragments(codes[:1000], k, n, 7, T)
    # the other genomes: whole copies, or windows that cover the sequence between them
    gen = mc.genomes(12, k, n, 7, T, span=60_000)
    total = int(lens.sum())
    assert [len(c) for c in gen[0]] == lens.tolist() and all(len(g) == 1 and len(g[0]) == 60_000 for g in gen[1:])
    base = po.synth_genomes(12, [total], 0.02, 7)
    assert gen[1][0] == po.codes_to_ascii(base[1][0][:60_000]) and gen[11][0] == po.codes_to_ascii(base[11][0][total - 60_000:])
    assert all(len(g[0]) == total for g in mc.genomes(3, k, n, 7, T)[1:])


def _read_fasta(tmp_path, text):
    p = tmp_path / "x.fa"
    p.write_bytes(text)
    return list(pidx.read_fasta(str(p)))


@pytest.mark.parametrize("width,crlf", [(1, False), (7, False), (60, False), (60, True)])
def test_fasta_readers_agree_on_the_fragmented_set(tmp_path, width, crlf):
    n, k = 3000, 21
    contigs = mc.genomes(1, k, n, 7, T)[0]
    text = mc.fasta(contigs, width, crlf)
    names, lens, offs = search.scan_fasta(text)
    assert names == mc.names_for(n) and lens.tolist() == [len(c) for c in contigs] and len(offs) == n + 1
    recs = _read_fasta(tmp_path, text)
    assert [r[0] for r in recs] == names and [r[1] for r in recs] == contigs
    assert (lens == 0).sum() > 300
    if crlf:
        assert text.count(b"\r\n") == text.count(b"\n") > n


@pytest.mark.parametrize("nheaders", mc.HEADER_COUNTS)
def test_fasta_readers_agree_on_the_text_of_many_headers(tmp_path, nheaders):
    text, names, seqs = mc.header_text(nheaders, 11)
    assert len(text) >= mc.BIG_TEXT and not text.endswith(b"\n")
    got_names, lens, offs = search.scan_fasta(text)
    assert len(got_names) == nheaders and got_names == names and lens.tolist() == [len(s) for s in seqs]
    recs = _read_fasta(tmp_path, text)
    assert [r[0] for r in recs] == names and [r[1] for r in recs] == seqs
    size = np.diff(offs)
    filled = lens > 0
    assert 40 <= size[filled][:-1].min() and size.max() <= 90
    assert (~filled).sum() > 600 and sum(b">" in s for s in seqs) > 1000
    assert all(text[o] == ord(">") and (o == 0 or text[o - 1] == ord("\n")) for o in offs[:-1].tolist())
    pick = mc.header_text_picks(text, offs, lens)
    assert len(pick) >= 2000 and pick[0] == 0 and pick[-1] == nheaders - 1
    straddling = [i for i in range(nheaders) if offs[i] // 4096 != (offs[i + 1] - 1) // 4096]
    assert len(straddling) > 1000 and set(straddling) <= set(pick)
    for e in np.flatnonzero(~filled).tolist():
        assert {max(e - 1, 0), min(e + 1, nheaders - 1)} <= set(pick)
