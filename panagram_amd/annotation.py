"""GFF annotation as ``panagram view`` reads it: the gene and annotation tracks the reference writes next to an anchor
genome's bitmaps (``panagram/index.py:615-651, 663-791``), with their tabix indexes written and read by this module.

* ``gff_records``  — the GFF's gene records and annotation records (exons, CDS, UTRs, ...), each annotation record named
  after its root gene by following ``Parent`` through the annotation IDs (``index.py:694-735``).
* ``write_track``  — a track as BGZF text (blocks cut at line ends, at most 65280 payload bytes each, then the EOF block)
  plus its ``.csi``: the CSI v1 index that htslib's ``tabix -C`` / ``pysam.tabix_index(..., 0, 1, 2, csi=True)`` writes
  (min_shift 14, depth 6, tabix "generic" meta: sequence, 1-based start and end in columns 1, 2, 3).  The layout follows the
  published CSIv1 / tabix specifications; no htslib is involved on either side.
* ``TabixTrack``   — the read side: the ``.csi`` parsed by our own reader, ``fetch(chrom, start, end)`` with the 0-based
  half-open region of ``pysam.TabixFile.fetch``.
"""
from __future__ import annotations

import bisect
import os
import re
import struct
import zlib
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import pandas as pd

GFF_NAMES = ["chr", "source", "type", "start", "end", "score", "strand", "phase", "attr"]
TABIX_COLS = ["chr", "start", "end", "type", "name"]  # anno track (index.py:54)
TABIX_TYPES = {"start": int, "end": int}
GENE_COLS = ["chr", "start", "end", "name"]           # gene track, then the counts of positions held by 1 and by N genomes

BGZF_BLOCK = 65280
CSI_MIN_SHIFT, CSI_DEPTH = 14, 6
_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


# ---------------------------------------------------------------------------
# GFF records
# ---------------------------------------------------------------------------
def gff_attr(attr: pd.Series, name: str) -> pd.Series:
    """the first ``name=value`` of every attribute string, ``name`` matched case-insensitively (index.py:663-667)"""
    return attr.str.extract(f"{re.escape(name)}=([^;]+)", flags=re.IGNORECASE)[0]


def read_gff(path: str) -> pd.DataFrame:
    df = pd.read_csv(path, sep="\t", comment="#", header=None, names=GFF_NAMES,
                     usecols=["chr", "type", "start", "end", "attr"], dtype={"chr": str, "type": str, "attr": str})
    df["attr"] = df["attr"].fillna("")
    df["id"] = gff_attr(df["attr"], "ID")
    return df


def _by_position(df: pd.DataFrame) -> pd.DataFrame:
    return df.sort_values(["chr", "start"], kind="stable").reset_index(drop=True)


def gff_records(path: str, gene_types: Sequence[str] = ("gene",), anno_types: Optional[Sequence[str]] = None,
                name_attr: str = "Name") -> Tuple[pd.DataFrame, pd.DataFrame, List[str]]:
    """(genes [chr start end name id], annos [chr start end type name], anno types present, sorted).

    Genes: the records whose type is in ``gene_types``, named by ``name_attr`` or else ``ID``.  Annotations: the records
    whose type is in ``anno_types`` — every non-gene record when that is None — without ``transcript`` records and without
    duplicate rows.  A record with a ``Parent`` is named after the gene at the root of its chain of parents (followed
    through the annotation records' IDs); a root record by its own ``name_attr`` / ``ID``.  A chain that ends in an ID that
    is not a gene keeps that ID as its name (the reference fails there)."""
    df = read_gff(path)
    gmask = df["type"].isin(list(gene_types))
    genes = _by_position(df[gmask])
    annos = _by_position(df[df["type"].isin(list(anno_types))] if anno_types is not None else df[~gmask])
    genes["name"] = gff_attr(genes["attr"], name_attr).fillna(genes["id"])

    parents = gff_attr(annos["attr"], "Parent").to_numpy(object)
    ids = annos["id"].to_numpy(object)
    row_of: Dict[str, int] = {}
    for i, x in enumerate(ids):
        if isinstance(x, str) and x not in row_of:  # (an ID shared by several records, as CDS pieces do: the first one)
            row_of[x] = i
    root = parents.copy()
    for i in range(len(root)):
        p, hops = root[i], 0
        while isinstance(p, str) and p in row_of and hops <= len(root):  # (a cycle of parents ends after len(annos) hops)
            nxt = parents[row_of[p]]
            if not isinstance(nxt, str):
                break
            p, hops = nxt, hops + 1
        root[i] = p
    gene_name = dict(zip(genes["id"].dropna(), genes.loc[genes["id"].notna(), "name"]))
    names = np.empty(len(annos), object)
    own = gff_attr(annos["attr"], name_attr).fillna(annos["id"]).to_numpy(object)
    for i, p in enumerate(root):
        names[i] = gene_name.get(p, p) if isinstance(p, str) else own[i]
    annos["name"] = names
    annos = annos[annos["type"] != "transcript"][TABIX_COLS].drop_duplicates().reset_index(drop=True)
    present = set(annos["type"].unique())
    types = sorted(present if anno_types is None else present.intersection(anno_types))
    return genes[["chr", "start", "end", "name", "id"]], annos, types


# ---------------------------------------------------------------------------
# BGZF text + CSI index (write side)
# ---------------------------------------------------------------------------
def _bgzf_block(payload: bytes, level: int = 6) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = c.compress(payload) + c.flush()
    bsize = 18 + len(body) + 8
    hdr = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", bsize - 1)
    return hdr + body + struct.pack("<II", zlib.crc32(payload) & 0xFFFFFFFF, len(payload))


def bgzf_compress(data: bytes, cuts: Optional[Sequence[int]] = None) -> Tuple[bytes, List[Tuple[int, int]]]:
    """``data`` as BGZF: blocks end at the offsets ``cuts`` allows (line ends), at most BGZF_BLOCK bytes each, then the EOF
    block.  Returns (file bytes, [(compressed offset, payload offset)] of every data block)."""
    if cuts is None:
        cuts = list(range(BGZF_BLOCK, len(data), BGZF_BLOCK))
    out, blocks, start, coff = [], [], 0, 0
    ends = [c for c in cuts if 0 < c < len(data)] + [len(data)]
    i = 0
    while start < len(data):
        # the last allowed cut within BGZF_BLOCK bytes; a line longer than a block is cut inside (BGZF allows it)
        j = bisect.bisect_right(ends, start + BGZF_BLOCK, lo=i) - 1
        end = ends[j] if j >= i and ends[j] > start else min(len(data), start + BGZF_BLOCK)
        i = max(i, j)
        blk = _bgzf_block(data[start:end])
        blocks.append((coff, start))
        out.append(blk)
        coff += len(blk)
        start = end
    out.append(_EOF)
    return b"".join(out), blocks


def reg2bin(beg: int, end: int, min_shift: int = CSI_MIN_SHIFT, depth: int = CSI_DEPTH) -> int:
    """the CSI bin of the 0-based half-open interval [beg, end) (CSIv1 specification, reg2bin)"""
    s, t = min_shift, ((1 << (depth * 3)) - 1) // 7
    end -= 1
    lvl = depth
    while lvl > 0:
        if beg >> s == end >> s:
            return t + (beg >> s)
        lvl -= 1
        s += 3
        t -= 1 << (lvl * 3)
    return 0


def reg2bins(beg: int, end: int, min_shift: int = CSI_MIN_SHIFT, depth: int = CSI_DEPTH) -> List[int]:
    """every bin that may hold a record overlapping [beg, end) (CSIv1 specification, reg2bins)"""
    if beg >= end:
        return []
    end -= 1
    s, t, out = min_shift + depth * 3, 0, []
    for lvl in range(depth + 1):
        out.extend(range(t + (beg >> s), t + (end >> s) + 1))
        s -= 3
        t += 1 << (lvl * 3)
    return out


def bin_first_pos(b: int, min_shift: int = CSI_MIN_SHIFT, depth: int = CSI_DEPTH) -> int:
    t, lvl = 0, 0
    while lvl < depth and b >= t + (1 << (lvl * 3)):
        t += 1 << (lvl * 3)
        lvl += 1
    return (b - t) << (min_shift + 3 * (depth - lvl))


def _interval(start: int, end: int) -> Tuple[int, int]:
    """a record's 0-based half-open interval: the generic format's start column is 1-based"""
    beg = max(0, int(start) - 1)
    return beg, max(int(end), beg + 1)


def csi_bytes(names: List[str], recs: List[Tuple[int, int, int, int, int]]) -> bytes:
    """The uncompressed CSI v1 index of records (ref, beg, end, voffset of the line, voffset behind it) in file order."""
    aux = struct.pack("<7i", 0, 1, 2, 3, ord("#"), 0, sum(len(n.encode()) + 1 for n in names))
    aux += b"".join(n.encode() + b"\0" for n in names)
    out = [b"CSI\x01", struct.pack("<3i", CSI_MIN_SHIFT, CSI_DEPTH, len(aux)), aux, struct.pack("<i", len(names))]
    by_ref: Dict[int, List[Tuple[int, int, int, int, int]]] = {}
    for r in recs:
        by_ref.setdefault(r[0], []).append(r)
    for ref in range(len(names)):
        rr = by_ref.get(ref, [])
        bins: Dict[int, List[List[int]]] = {}
        for _, beg, end, v0, v1 in rr:
            ch = bins.setdefault(reg2bin(beg, end), [])
            if ch and ch[-1][1] == v0:  # the next line of the same bin: the chunk grows
                ch[-1][1] = v1
            else:
                ch.append([v0, v1])
        # loffset: the first record of the ref (file order) whose end lies past the bin's first position
        run_max = np.maximum.accumulate(np.array([r[2] for r in rr], np.int64)) if rr else np.zeros(0, np.int64)
        out.append(struct.pack("<i", len(bins)))
        for b in sorted(bins):
            i = int(np.searchsorted(run_max, bin_first_pos(b), side="right"))
            loff = rr[min(i, len(rr) - 1)][3]
            out.append(struct.pack("<IQi", b, loff, len(bins[b])))
            out.extend(struct.pack("<QQ", c0, c1) for c0, c1 in bins[b])
    return b"".join(out)


def write_track(path: str, df: pd.DataFrame) -> None:
    """``df`` (first three columns: chr, 1-based start, end; sorted by chr then start) as tab-separated BGZF text at
    ``path`` plus ``path + '.csi'``; both written to temporaries and renamed."""
    lines = df.to_csv(sep="\t", header=False, index=False, lineterminator="\n").encode()
    ends = np.flatnonzero(np.frombuffer(lines, np.uint8) == 10) + 1 if lines else np.zeros(0, np.int64)
    gz, blocks = bgzf_compress(lines, ends.tolist())
    bc = np.array([b[0] for b in blocks], np.int64)
    bu = np.array([b[1] for b in blocks] + [len(lines)], np.int64)

    def voff(u: int) -> int:  # payload offset -> virtual offset (a block's end = the next block's start)
        i = int(np.searchsorted(bu, u, side="right")) - 1
        if i >= len(bc):
            return (len(gz) - len(_EOF)) << 16
        return (int(bc[i]) << 16) | (u - int(bu[i]))
    names: List[str] = []
    ref_of: Dict[str, int] = {}
    recs = []
    starts = np.concatenate([[0], ends[:-1]]) if len(ends) else np.zeros(0, np.int64)
    for (chrom, st, en), u0, u1 in zip(df.iloc[:, :3].itertuples(index=False, name=None), starts.tolist(), ends.tolist()):
        chrom = str(chrom)
        if chrom not in ref_of:
            ref_of[chrom] = len(names)
            names.append(chrom)
        beg, end = _interval(st, en)
        recs.append((ref_of[chrom], beg, end, voff(u0), voff(u1)))
    csi, _ = bgzf_compress(csi_bytes(names, recs))
    for p, data in ((path, gz), (path + ".csi", csi)):
        with open(p + ".tmp", "wb") as f:
            f.write(data)
    os.replace(path + ".tmp", path)
    os.replace(path + ".csi.tmp", path + ".csi")


# ---------------------------------------------------------------------------
# read side
# ---------------------------------------------------------------------------
def read_bgzf(path: str) -> Tuple[bytes, np.ndarray, np.ndarray]:
    """(payload, compressed offsets, payload offsets) of every block of a BGZF file, walked through BSIZE"""
    raw = open(path, "rb").read()
    out, co, uo, off, u = [], [], [], 0, 0
    while off < len(raw):
        if raw[off:off + 4] != b"\x1f\x8b\x08\x04" or off + 18 > len(raw):
            raise ValueError(f"{path}: not a BGZF block at offset {off}")
        xlen = struct.unpack_from("<H", raw, off + 10)[0]
        bsize, i = None, off + 12
        while i + 4 <= off + 12 + xlen:
            si, slen = raw[i:i + 2], struct.unpack_from("<H", raw, i + 2)[0]
            if si == b"BC" and slen == 2:
                bsize = struct.unpack_from("<H", raw, i + 4)[0] + 1
            i += 4 + slen
        if bsize is None:
            raise ValueError(f"{path}: BGZF block at offset {off} has no BSIZE")
        data = zlib.decompress(raw[off + 12 + xlen:off + bsize - 8], -15)
        co.append(off)
        uo.append(u)
        out.append(data)
        u += len(data)
        off += bsize
    return b"".join(out), np.array(co, np.int64), np.array(uo, np.int64)


class TabixTrack:
    """A BGZF track and its ``.csi``, read by our own code: ``fetch(chrom, start, end)`` gives the lines (as lists of
    fields) of the records overlapping the 0-based half-open region, in file order — what pysam.TabixFile.fetch gives."""

    def __init__(self, path: str, index: Optional[str] = None):
        self.text, co, uo = read_bgzf(path)
        self._u_of = dict(zip(co.tolist(), uo.tolist()))
        idx, _, _ = read_bgzf(index or path + ".csi")
        if idx[:4] != b"CSI\x01":
            raise ValueError(f"{index or path + '.csi'}: not a CSI index")
        self.min_shift, self.depth, l_aux = struct.unpack_from("<3i", idx, 4)
        aux = idx[16:16 + l_aux]
        fmt, self.col_seq, self.col_beg, self.col_end, meta, skip, l_nm = struct.unpack_from("<7i", aux, 0)
        self.names = [n.decode() for n in aux[28:28 + l_nm].split(b"\0")[:-1]]
        p = 16 + l_aux
        (n_ref,) = struct.unpack_from("<i", idx, p)
        p += 4
        self.bins: List[Dict[int, Tuple[int, List[Tuple[int, int]]]]] = []
        for _ in range(n_ref):
            (n_bin,) = struct.unpack_from("<i", idx, p)
            p += 4
            bins = {}
            for _ in range(n_bin):
                b, loff, n_chunk = struct.unpack_from("<IQi", idx, p)
                p += 16
                ch = [struct.unpack_from("<QQ", idx, p + 16 * j) for j in range(n_chunk)]
                p += 16 * n_chunk
                bins[b] = (loff, ch)
            self.bins.append(bins)
        self._ref = {n: i for i, n in enumerate(self.names)}

    def _u(self, v: int) -> int:
        return self._u_of[v >> 16] + (v & 0xFFFF)

    def _lines(self, u0: int, u1: int) -> Iterator[List[str]]:
        for line in self.text[u0:u1].decode().splitlines():
            if line and not line.startswith("#"):
                yield line.split("\t")

    def fetch(self, chrom: Optional[str] = None, start: Optional[int] = None, end: Optional[int] = None) -> List[List[str]]:
        if chrom is None:
            return list(self._lines(0, len(self.text)))
        if chrom not in self._ref:
            return []
        beg = 0 if start is None else max(0, int(start))
        stop = (1 << (self.min_shift + 3 * self.depth)) if end is None else int(end)
        bins = self.bins[self._ref[chrom]]
        chunks = sorted(c for b in reg2bins(beg, stop, self.min_shift, self.depth) if b in bins for c in bins[b][1])
        out, done = [], -1
        for v0, v1 in chunks:
            u0, u1 = self._u(v0), self._u(v1)
            if u1 <= done:
                continue
            u0 = max(u0, done)
            for f in self._lines(u0, u1):
                b_, e_ = _interval(int(f[self.col_beg - 1]), int(f[self.col_end - 1]))
                if f[self.col_seq - 1] == chrom and b_ < stop and e_ > beg:
                    out.append(f)
            done = u1
        return out


def gene_track(genes: pd.DataFrame, occ1: np.ndarray, occn: np.ndarray, ngenomes: int) -> pd.DataFrame:
    """the gene track's rows: chr start end name, then the gene's positions held by 1 genome and by all N.  Every GFF gene
    is one row with its own counts (the reference adds a duplicate gene's counts twice into one row; not copied)."""
    df = genes[GENE_COLS].copy()
    df[1] = np.asarray(occ1, np.int64)
    df[ngenomes] = np.asarray(occn, np.int64)
    return df.sort_values(["chr", "start"], kind="stable").reset_index(drop=True)
