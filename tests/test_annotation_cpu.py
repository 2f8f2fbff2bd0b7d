"""CPU: GFF records, and the BGZF + CSI tracks written and read back by panagram_amd.annotation — checked by the CSIv1 /
tabix specifications (bins recomputed here with the spec's reg2bin) and by brute-force overlap queries."""
import gzip
import struct
import zlib

import numpy as np
import pandas as pd
import pytest

from panagram_amd import annotation as an

GFF = """##gff-version 3
chr2\tsrc\tgene\t500\t900\t.\t+\t.\tID=geneB;Name=Beta
chr1\tsrc\tgene\t100\t400\t.\t+\t.\tID=geneA
chr1\tsrc\tmRNA\t100\t400\t.\t+\t.\tID=txA;Parent=geneA
chr1\tsrc\ttranscript\t100\t400\t.\t+\t.\tID=trA;Parent=geneA
chr1\tsrc\texon\t100\t200\t.\t+\t.\tID=exA1;parent=txA
chr1\tsrc\tCDS\t120\t200\t.\t+\t0\tParent=txA
chr1\tsrc\tCDS\t120\t200\t.\t+\t0\tParent=txA
chr2\tsrc\texon\t500\t600\t.\t+\t.\tParent=geneB
chr2\tsrc\trepeat\t50\t60\t.\t+\t.\tID=rep1;Name=Alu1
chr2\tsrc\trepeat\t70\t80\t.\t+\t.\tID=rep2
"""


def test_gff_records(tmp_path):
    p = tmp_path / "a.gff"
    p.write_text(GFF)
    genes, annos, types = an.gff_records(str(p))
    assert genes[["chr", "start", "end", "name"]].values.tolist() == [["chr1", 100, 400, "geneA"], ["chr2", 500, 900, "Beta"]]
    rows = annos.values.tolist()
    assert ["chr1", 100, 400, "transcript", "geneA"] not in rows  # transcript dropped
    assert rows.count(["chr1", 120, 200, "CDS", "geneA"]) == 1      # duplicates dropped
    assert ["chr1", 100, 200, "exon", "geneA"] in rows              # two parents deep, `parent=` matched case-insensitively
    assert ["chr2", 500, 600, "exon", "Beta"] in rows
    assert ["chr2", 50, 60, "repeat", "Alu1"] in rows and ["chr2", 70, 80, "repeat", "rep2"] in rows  # roots: Name, else ID
    assert types == ["CDS", "exon", "mRNA", "repeat"]
    assert annos.sort_values(["chr", "start"], kind="stable").values.tolist() == rows
    _, annos2, types2 = an.gff_records(str(p), anno_types=["exon", "CDS", "UTR"])
    assert set(annos2["type"]) == {"exon", "CDS"} and types2 == ["CDS", "exon"]
    g3, _, _ = an.gff_records(str(p), gene_types=["gene", "mRNA"], name_attr="ID")
    assert g3["name"].tolist() == ["geneA", "txA", "geneB"]


def spec_reg2bin(beg, end, min_shift=14, depth=6):
    end -= 1
    for lvl, s in ((6, 14), (5, 17), (4, 20), (3, 23), (2, 26), (1, 29)):
        if beg >> s == end >> s:
            return ((1 << (3 * lvl)) - 1) // 7 + (beg >> s)
    return 0


def blocks_of(raw):
    out, off = [], 0
    while off < len(raw):
        bsize = struct.unpack_from("<H", raw, off + 16)[0] + 1
        data = zlib.decompress(raw[off + 18:off + bsize - 8], -15)
        out.append((off, data))
        off += bsize
    return out


def random_track(rng):
    chroms = {"chrA": 5_000_000, "chrB": 40_000, "chrLong": (1 << 29) + 3_000_000, "chrC": 300}
    recs = []
    for c, L in chroms.items():
        n = 3000 if c != "chrC" else 5
        st = rng.integers(1, L, n)
        ln = np.where(rng.random(n) < 0.05, rng.integers(1, 2_000_000, n), rng.integers(1, 5000, n))
        for s, l in zip(st, ln):
            recs.append((c, int(s), int(s + l), "exon", f"g{len(recs)}"))
    df = pd.DataFrame(recs, columns=an.TABIX_COLS)
    return df.sort_values(["chr", "start"], kind="stable").reset_index(drop=True), chroms


def test_track_round_trip(tmp_path):
    rng = np.random.default_rng(7)
    df, chroms = random_track(rng)
    path = str(tmp_path / "anno.bed.gz")
    an.write_track(path, df)
    raw = open(path, "rb").read()
    blocks = blocks_of(raw)
    # every block ends at a line end, none holds more than 65280 bytes, the file ends with the EOF block
    assert raw.endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    assert all(d.endswith(b"\n") and len(d) <= 65280 for _, d in blocks[:-1]) and blocks[-1][1] == b""
    text = gzip.decompress(raw)
    lines = text.decode().splitlines()
    assert lines == [("\t".join(map(str, r))) for r in df.itertuples(index=False, name=None)]
    # the test's own walk of the index: header, aux, and every record's bin listing its chunk
    idx = gzip.decompress(open(path + ".csi", "rb").read())
    assert idx[:4] == b"CSI\x01"
    min_shift, depth, l_aux = struct.unpack_from("<3i", idx, 4)
    assert (min_shift, depth) == (14, 6)
    fmt, cs, cb, ce, meta, skip, l_nm = struct.unpack_from("<7i", idx, 16)
    assert (fmt, cs, cb, ce, chr(meta), skip) == (0, 1, 2, 3, "#", 0)
    names = idx[16 + 28:16 + 28 + l_nm].split(b"\0")[:-1]
    assert [n.decode() for n in names] == list(dict.fromkeys(df["chr"]))
    p = 16 + l_aux
    n_ref = struct.unpack_from("<i", idx, p)[0]
    p += 4
    bins = []
    for _ in range(n_ref):
        nb = struct.unpack_from("<i", idx, p)[0]
        p += 4
        d = {}
        for _ in range(nb):
            b, loff, nc = struct.unpack_from("<IQi", idx, p)
            p += 16
            d[b] = [struct.unpack_from("<QQ", idx, p + 16 * j) for j in range(nc)]
            p += 16 * nc
        bins.append(d)
    co = [o for o, _ in blocks]
    uo = np.concatenate([[0], np.cumsum([len(d) for _, d in blocks])])
    to_u = lambda v: int(uo[co.index(v >> 16)]) + (v & 0xFFFF)  # noqa: E731
    line_starts = set(np.concatenate([[0], np.flatnonzero(np.frombuffer(text, np.uint8) == 10) + 1]).tolist())
    u = 0
    ref_of = {n.decode(): i for i, n in enumerate(names)}
    for line in lines:
        c, s, e = line.split("\t")[:3]
        beg, end = int(s) - 1, int(e)
        b = spec_reg2bin(beg, end)
        chunks = bins[ref_of[c]][b]
        assert any(to_u(c0) <= u and u + len(line) + 1 <= to_u(c1) for c0, c1 in chunks), line
        u += len(line) + 1
    for d in bins:
        for chunks in d.values():
            for c0, c1 in chunks:
                assert to_u(c0) in line_starts and to_u(c1) in line_starts  # no chunk crosses a line
    # queries against brute force over the inflated text
    t = an.TabixTrack(path)
    arr = df.to_numpy(object)
    for _ in range(2000):
        c = list(chroms)[int(rng.integers(0, len(chroms)))]
        a = int(rng.integers(0, chroms[c]))
        b = a + int(rng.integers(1, 3_000_000 if rng.random() < 0.1 else 20_000))
        want = [list(map(str, r)) for r in arr if r[0] == c and r[1] - 1 < b and r[2] > a]
        assert t.fetch(c, a, b) == want, (c, a, b)
    assert t.fetch("chrNone", 0, 10) == []
    assert len(t.fetch()) == len(df)
    try:
        import pysam
    except ImportError:
        pysam = None
    if pysam is not None:
        tf = pysam.TabixFile(path, index=path + ".csi", parser=pysam.asTuple())
        for c in chroms:
            assert [list(r) for r in tf.fetch(c, 0, 1000)] == t.fetch(c, 0, 1000)


def test_pysam_reads_the_track(tmp_path):
    pysam = pytest.importorskip("pysam")
    df, _ = random_track(np.random.default_rng(1))
    path = str(tmp_path / "g.bed.gz")
    an.write_track(path, df)
    tf = pysam.TabixFile(path, index=path + ".csi", parser=pysam.asTuple())
    t = an.TabixTrack(path)
    for c, a, b in (("chrA", 0, 10 ** 6), ("chrLong", 1 << 29, (1 << 29) + 10 ** 6), ("chrB", 100, 200)):
        assert [list(r) for r in tf.fetch(c, a, b)] == t.fetch(c, a, b)


def test_reg2bin_matches_spec():
    rng = np.random.default_rng(2)
    for _ in range(5000):
        a = int(rng.integers(0, 1 << 31))
        b = a + int(rng.integers(1, 1 << int(rng.integers(1, 30))))
        b = min(b, 1 << 32)
        assert an.reg2bin(a, b) == spec_reg2bin(a, b)
        assert an.reg2bin(a, b) in an.reg2bins(a, b)
