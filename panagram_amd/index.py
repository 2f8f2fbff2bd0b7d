"""Host-side counterpart of the reference's write path (``panagram/index.py``), scoped to
the anchor hot path and driving the HIP kernels through the C-ABI.

Mirrors, with the same names / argument meaning / on-disk layout:

* ``Index``  — config + orchestration (``panagram/index.py:85-466``): ``samples.tsv``
  schema ``name fasta gff id anchor`` (``:269-295``), ``config.yaml`` keys (``:347-357``),
  ``kmc_bitvec_count`` / ``bitvec_prefixes`` / ``steps`` (``:391-405``), ``run()``.
  Where the reference launches Snakemake -> kmc -> kmc_tools -> one anchor job per genome,
  ``Index.run()`` builds the pan-kmer table on the GPU (or loads existing
  ``kmc/bitvec{i}.kmc_{pre,suf}``) and anchors every anchor genome in-process.
* ``Genome`` — ``run_anchor`` (``:1012-1097``), ``iter_fasta`` (``:922-930``),
  ``set_chrs`` offsets (``:596-604``) and the read side ``load_bgz_blocks`` /
  ``_query_bytes`` / ``query`` (``:793-845``) so that what we write can be read back the way
  ``panagram view`` reads it.

Output tree (identical to the reference's):
    <prefix>/config.yaml, samples.tsv
    <prefix>/anchor/<name>/bitmap.1.gz(.gzi) bitmap.100.gz(.gzi) bitsum.bins.tsv chrs.tsv
                           total_paircounts.csv

    <prefix>/genome_dist.tsv       (opt-in: ``genome_dist=True`` / ``index --genome_dist`` / the ``dist`` command;
                                    MinHash sketches taken on the GPU in place of `mash sketch` + `mash triangle`)
    <prefix>/anchor/<name>/gene.bed.gz(.csi) anno.bed.gz(.csi) anno_types.txt
                                   (opt-in: ``annotate=True`` / ``index --annotate`` / the ``annotate`` command:
                                    ``Genome.run_annotate``, index.py:971-1010; bitmap.1.gz inflated on the GPU)

    <prefix>/anchor/<name>/chrom_umaps.csv genome_umap.csv
                                   (opt-in: ``umaps=True`` / ``index --umaps`` / the ``umaps`` command: ``Genome.write_umaps``,
                                    index.py:1107-1156; exact neighbours on the GPU, the layout restated in ``umap.py`` —
                                    the files' layout is the reference's, umap-learn's numbers are not claimed)

Out of scope here: mash's own .msh files, the viewer.
"""
from __future__ import annotations

import dataclasses
import gzip
import logging
import os
import re
import struct
import zlib
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import pandas as pd
import yaml

from . import engine

logger = logging.getLogger(__name__)

NAME_REGEX = "[A-Za-z0-9_-]+"
BGZ_SUFFIX = "gz"
IDX_SUFFIX = "gzi"
ANCHOR_DIR = "anchor"
_WS = b" \t\r\n\x0b\x0c"


# ---------------------------------------------------------------------------
# FASTA
# ---------------------------------------------------------------------------
def read_fasta(path: str) -> Iterator[Tuple[str, bytes]]:
    """Yield ``(record id, sequence bytes)``.  Semantics of the reference's Python path
    (``Bio.SeqIO`` via ``iter_fasta``, index.py:922-930): id = header up to the first
    whitespace, sequence lines joined with all whitespace removed, ``.gz``/``.bgz`` read
    through gzip.  (The C++ variant keeps ``\\r`` bytes in the sequence, cpp/anchor.cpp:77-93;
    the two agree on well-formed FASTA.)"""
    opn = gzip.open if path.endswith((".gz", ".bgz")) else open
    with opn(path, "rb") as f:
        data = f.read()
    pos = 0 if data[:1] == b">" else data.find(b"\n>") + 1
    if pos == 0 and data[:1] != b">":
        return
    n = len(data)
    while pos < n:
        eol = data.find(b"\n", pos)
        if eol < 0:
            eol = n
        header = data[pos + 1:eol].strip()
        nxt = data.find(b"\n>", eol)
        end = n if nxt < 0 else nxt + 1
        seq = data[eol + 1:end].translate(None, _WS)
        name = header.split(None, 1)[0].decode("latin-1") if header else ""
        yield name, seq
        pos = end


FASTQ_SUFFIXES = (".fastq", ".fastq.gz", ".fq", ".fq.gz")  # workflow/Snakefile:88-89


def _read_fasta_image(path: str) -> np.ndarray:
    """the bytes of a FASTA file (``.gz`` / ``.bgz`` inflated) for ``SeqSet.from_fasta``"""
    if path.endswith((".gz", ".bgz")):
        import gzip
        with gzip.open(path, "rb") as f:
            return np.frombuffer(f.read(), dtype=np.uint8)
    return np.fromfile(path, dtype=np.uint8)


class _PinnedPool:
    """up to ``budget`` page-locked buffers of ``cap`` bytes (engine.HostBuffer) that go round between the reader threads and
    the thread that uploads their contents; a reader locks the memory of a new one itself (in parallel with the others' reads)
    as long as the budget is not spent.  ``get()`` returns None once locking memory has failed: read into pageable memory."""

    def __init__(self, make, cap: int, budget: int):
        import queue
        import threading
        self.make, self.cap, self.budget = make, cap, budget
        self.free, self.lock, self.made, self.failed, self.all = queue.Queue(), threading.Lock(), 0, False, []

    def get(self):
        import queue
        try:
            return self.free.get_nowait()
        except queue.Empty:
            pass
        with self.lock:
            create = not self.failed and self.made < self.budget
            if create:
                self.made += 1
        if create:
            try:
                buf = self.make(self.cap)
            except Exception:  # noqa: BLE001 — no memory to lock
                with self.lock:
                    self.made -= 1
                    self.failed = True
                return None
            with self.lock:
                self.all.append(buf)
            return buf
        if self.failed:  # (fewer buffers than files in flight: waiting for one could wait for a LATER file's, which is handed on only after this one)
            return None
        return self.free.get()

    def put(self, buf) -> None:
        self.free.put(buf)

    def close(self) -> None:
        for b in self.all:
            b.close()
        self.all = []


def _read_fasta_pinned(path: str, pool: _PinnedPool):
    """a plain FASTA file read into a page-locked buffer of ``pool``: ``(uint8 view of the text, the buffer)`` — the caller puts
    the buffer back once the text is on the device; compressed files, and any file when no memory can be locked, as
    ``_read_fasta_image`` reads them: ``(image, None)``"""
    if path.endswith((".gz", ".bgz")):
        return _read_fasta_image(path), None
    buf = pool.get()
    if buf is None:
        return _read_fasta_image(path), None
    try:
        n = 0
        with open(path, "rb", buffering=0) as f:
            view = memoryview(buf.array)
            while n < len(view):
                got = f.readinto(view[n:])
                if not got:
                    break
                n += got
            if n == len(view) and f.read(1):  # (the file grew since it was sized)
                raise OSError(f"{path} is larger than when the index was prepared")
        return buf.array[:n], buf
    except BaseException:
        pool.put(buf)
        raise


def is_fastq(path) -> bool:
    return isinstance(path, str) and path.endswith(FASTQ_SUFFIXES)


def read_fastq_joined(path: str) -> bytes:
    """The reads of a 4-line-record FASTQ joined by ``N``: no k-mer window spans two reads, which is
    how kmc -fq counts them."""
    opn = gzip.open if path.endswith(".gz") else open
    with opn(path, "rb") as f:
        lines = f.read().split(b"\n")
    return b"N".join(ln.rstrip(b"\r") for ln in lines[1::4])


# ---------------------------------------------------------------------------
# KMC1 database files (format: SURVEY.md Appendix A) — writer, so that tables built on
# the GPU can be handed to the reference (`kmc/bitvec{i}.kmc_pre|.kmc_suf`)
# ---------------------------------------------------------------------------
def write_kmc1(prefix: str, keys: np.ndarray, counters: np.ndarray, k: int,
               lut_prefix_len: Optional[int] = None) -> None:
    keys = np.ascontiguousarray(keys, np.uint64)
    counters = np.ascontiguousarray(counters, np.uint32)
    order = np.argsort(keys, kind="stable")
    keys, counters = keys[order], counters[order]
    if lut_prefix_len is None:
        cands = [p for p in range(1, min(k, 13)) if (k - p) % 4 == 0]
        lut_prefix_len = cands[0]
        for p in cands:
            if 4 ** p <= max(len(keys), 1) * 4:
                lut_prefix_len = p
    p = lut_prefix_len
    if (k - p) % 4:
        raise ValueError("(k - lut_prefix_len) must be a multiple of 4")
    suf_bytes = (k - p) // 4
    pref = (keys >> np.uint64(2 * (k - p))).astype(np.int64)
    lut = np.searchsorted(pref, np.arange(4 ** p, dtype=np.int64), side="left").astype(np.uint64)
    with open(prefix + ".kmc_pre", "wb") as f:
        f.write(b"KMCP")
        f.write(lut.tobytes())
        f.write(struct.pack("<IIIIIIQB3x24xI", k, 0, 4, p, 1, 0xFFFFFFFF, len(keys), 0, 0))
        f.write(struct.pack("<I", 64))
        f.write(b"KMCP")
    rec = np.zeros((len(keys), suf_bytes + 4), np.uint8)
    for b in range(suf_bytes):
        rec[:, b] = ((keys >> np.uint64(8 * (suf_bytes - 1 - b))) & np.uint64(0xFF)).astype(np.uint8)
    rec[:, suf_bytes:] = counters.view(np.uint8).reshape(-1, 4)
    with open(prefix + ".kmc_suf", "wb") as f:
        f.write(b"KMCS")
        f.write(rec.tobytes())
        f.write(b"KMCS")


# ---------------------------------------------------------------------------
# BGZF read side (Bio.bgzf is not a dependency here)
# ---------------------------------------------------------------------------
def load_bgz_blocks(fname: str) -> np.ndarray:
    """index.py:793-799: (rstart, dstart) per block, block 0 implicit."""
    raw = np.fromfile(fname, "<u8")
    n = int(raw[0])
    blocks = np.zeros((n + 1, 2), np.int64)
    blocks[1:] = raw[1:1 + 2 * n].reshape(n, 2)
    return blocks


def bgzf_read(path: str, blocks: np.ndarray, byte_start: int, length: int) -> bytes:
    """Random access as in index.py:827-845: locate the block through the .gzi, then inflate."""
    blk = int(np.searchsorted(blocks[:, 1], byte_start, side="right") - 1)
    out = bytearray()
    skip = byte_start - int(blocks[blk, 1])
    with open(path, "rb") as f:
        f.seek(int(blocks[blk, 0]))
        while len(out) < length:
            hdr = f.read(18)
            if len(hdr) < 18:
                break
            bsize = struct.unpack("<H", hdr[16:18])[0] + 1
            body = f.read(bsize - 18)
            data = zlib.decompress(body[:-8], -15)
            if not data:
                break  # EOF block
            out += data[skip:]
            skip = 0
    return bytes(out[:length])


# ---------------------------------------------------------------------------
# config dataclasses (same field names and defaults as index.py:63-138)
# ---------------------------------------------------------------------------
@dataclasses.dataclass
class KMC:
    memory: int = 8
    threads: int = 1
    use_existing: bool = False


@dataclasses.dataclass
class UMAP:
    neighbors: int = 4
    dist: float = 0
    eps: float = 1
    samples: int = 1
    bin_size: int = 100000


# ---------------------------------------------------------------------------
# the tree of the genomes over a region, from their pair counts (view.py:576-596, 751-764)
# ---------------------------------------------------------------------------
def linkage_newick(Z: np.ndarray, names: Sequence[str]) -> str:
    """A scipy linkage matrix as Newick text in the convention of the viewer's trees (view.py:576-596): leaves ``name:%.2f``,
    a branch's length its parent's height minus its own, a node's second child written before its first, the root closed
    with ``);``.  Built bottom-up over the rows of ``Z`` (no recursion: a tree of one long chain is as deep as N)."""
    n = len(names)
    if n == 1:
        return "(%s:%.2f);" % (names[0], 0.0)
    text, height = {i: str(names[i]) for i in range(n)}, {i: 0.0 for i in range(n)}
    for k, (a, b, h, _) in enumerate(np.asarray(Z, np.float64)):
        a, b = int(a), int(b)
        text[n + k] = "(%s:%.2f,%s:%.2f)" % (text.pop(b), h - height[b], text.pop(a), h - height[a])
        height[n + k] = float(h)
    return text[2 * n - 2] + ";"


def linkage_order(Z: np.ndarray, n: int) -> List[int]:
    """leaf numbers in dendrogram order (a node's first child before its second: scipy's ``leaves_list``)"""
    out, todo = [], [2 * n - 2] if n > 1 else [0]
    while todo:
        i = todo.pop()
        if i < n:
            out.append(i)
        else:
            todo += [int(Z[i - n, 1]), int(Z[i - n, 0])]
    return out


@dataclasses.dataclass
class RegionTree:
    """What ``Index.region_tree`` returns.  ``counts``: the pair counts C (N x N frame); ``distance``: the Hamming distances
    H = C[a][a] + C[b][b] - 2 C[a][b] (integers; sqrt(H) is the Euclidean distance of the two 0/1 columns); ``linkage``:
    scipy's Ward linkage of sqrt(H), equal to ``linkage(bitmap.T, "ward", "euclidean")``; ``order``: the leaf names in
    dendrogram order; ``shared_pct``: diag(C) / max(diag(C)) * 100, the viewer's kmer_num (zeros when no row holds a bit);
    ``newick``: the tree as text."""
    counts: pd.DataFrame
    distance: pd.DataFrame
    linkage: np.ndarray
    order: List[str]
    shared_pct: pd.Series
    newick: str

    @classmethod
    def from_counts(cls, counts, names: Sequence[str]) -> "RegionTree":
        names = list(names)
        n = len(names)
        C = np.asarray(counts, np.int64).reshape(n, n)
        d = np.diag(C)
        H = d[:, None] + d[None, :] - 2 * C
        if n > 1:
            try:
                from scipy.cluster.hierarchy import linkage
            except ImportError as e:
                raise ImportError("region_tree needs scipy for the Ward linkage (pair_counts does not)") from e
            Z = linkage(np.sqrt(H[np.triu_indices(n, 1)].astype(np.float64)), method="ward")
        else:
            Z = np.zeros((0, 4))
        idx = pd.Index(names)
        top = int(d.max()) if n else 0
        pct = d / top * 100.0 if top > 0 else np.zeros(n)
        return cls(counts=pd.DataFrame(C, index=idx, columns=idx), distance=pd.DataFrame(H, index=idx, columns=idx), linkage=Z,
                   order=[names[i] for i in linkage_order(Z, n)], shared_pct=pd.Series(pct, index=idx),
                   newick=linkage_newick(Z, names))


class _KmerStatsSwitch:
    """What ``Index.kmer_stats`` reads as: the switch ``Index(kmer_stats=True)`` set (its truth value) and, called, the
    pan-genome's k-mer statistics (``Index._kmer_stats_frames``) — one name for both, as the command line has one."""

    def __init__(self, index, on: bool):
        self._index, self._on = index, bool(on)

    def __bool__(self):
        return self._on

    def __call__(self):
        return self._index._kmer_stats_frames()

    def __deepcopy__(self, memo):  # (dataclasses.asdict: the switch alone)
        return self._on

    def __repr__(self):
        return repr(self._on)


class _KmerStatsField:
    """the dataclass field behind ``Index.kmer_stats``: stores the switch, reads as a _KmerStatsSwitch"""

    def __get__(self, obj, owner=None):
        if obj is None:
            return False  # (the field's default)
        return _KmerStatsSwitch(obj, obj.__dict__.get("_kmer_stats_on", False))

    def __set__(self, obj, value):
        obj.__dict__["_kmer_stats_on"] = bool(value)


@dataclasses.dataclass
class Index:
    """Anchor k-mer bitvectors to reference FASTA files to create the pan-kmer bitmap."""

    input: str
    mode: Optional[str] = None
    prefix: Optional[str] = None
    k: int = 21
    cores: int = 1
    lowres_step: int = 100
    max_bin_kbp: int = 200
    min_bin_count: int = 100
    max_view_chrs: int = 50
    gff_gene_types: List[str] = dataclasses.field(default_factory=lambda: ["gene"])
    gff_anno_types: Optional[List[str]] = None
    gff_name: str = "Name"
    anchor_genomes: Optional[List[str]] = None
    prepare: bool = False
    kmc: KMC = dataclasses.field(default_factory=KMC)
    genome_umap: UMAP = dataclasses.field(default_factory=UMAP)
    chrom_umap: UMAP = dataclasses.field(default_factory=UMAP)
    use_existing: int = 1
    threads: int = 1
    memory: int = 1
    # -- not part of the reference's schema: which GPU this process drives, and whether to
    #    also export kmc/bitvec{i} in KMC1 layout for the reference to read
    device: int = 0
    export_kmc: bool = False
    rank: int = dataclasses.field(default_factory=lambda: int(os.environ.get("RANK", "0")))
    world: int = dataclasses.field(default_factory=lambda: int(os.environ.get("WORLD_SIZE", "1")))

    # how a multi-process run divides the work (see run()): None = decide from the table's size
    shard: Optional[str] = dataclasses.field(default_factory=lambda: os.environ.get("PG_SHARD") or None)
    genome_blocks: int = dataclasses.field(default_factory=lambda: int(os.environ.get("PG_GENOME_BLOCKS", "0")))
    # build the replicated table from the genomes this process anchors, the other samples only set bits (PG_FULL_TABLE=1: all k-mers)
    filtered_table: bool = dataclasses.field(default_factory=lambda: os.environ.get("PG_FULL_TABLE", "") in ("", "0"))
    # also write genome_dist.tsv (write_genome_dist): off by default, so that the default tree and config.yaml stay as they were
    genome_dist: bool = False
    # run Genome.run_annotate() for every annotated anchor genome this process completes (off by default: the default tree
    # stays as it was)
    annotate: bool = False
    # run Genome.write_umaps() for every anchor genome this process completes (off by default: the default tree stays as it was)
    umaps: bool = False
    # build the table from every sample's k-mers and write kmer_shared.tsv and kmer_occupancy.tsv after the table build
    # (write_kmer_stats; off by default: the default tree stays as it was).  Called, ``kmer_stats()`` returns the frames.
    kmer_stats: bool = _KmerStatsField()

    _EXTRA = ("device", "export_kmc", "rank", "world", "shard", "genome_blocks", "filtered_table", "genome_dist", "annotate",
              "umaps", "kmer_stats")
    # keys of config.yaml that describe one invocation, not the index: not taken over when a directory is re-opened
    # (`prepare` is written for schema compatibility, but a later `index <dir>` run must not stop at "Prepared")
    _NOT_IN_CONFIG = ("input", "mode", "prefix", "prepare")
    SAMPLE_COLUMNS = ("fasta", "gff", "id", "anchor")  # after the index column `name` (index.py:282-293)

    # ---- opening an index: three ways in (index.py:196-268), one handler each ----
    def __post_init__(self):
        if self.mode not in (None, "r", "w"):
            raise ValueError(f"Invalid mode '{self.mode}', must be 'r' or 'w'")
        kind = "dir" if os.path.isdir(self.input) else "file" if os.path.isfile(self.input) else None
        self.write_mode = kind == "file" if self.mode is None else self.mode == "w"
        opener = {(True, "dir"): self._reopen_prepared, (True, "file"): self._create_from_samples,
                  (False, "dir"): self._open_readonly}.get((self.write_mode, kind))
        if opener is None:
            raise ValueError("Index input must be sample TSV or initialized directory" if self.write_mode
                             else "Index input must be directory mode='r'")
        opener()
        self._check_geometry()  # (after the config file has had its say)
        self._load_samples()
        self._ctx = None
        self._table = None
        self._table_scope = "all"
        self.timings: Dict[str, float] = {}  # seconds spent in load_inputs / build_table (host wall clock), for reports
        self._seqsets: Dict[str, engine.SeqSet] = {}
        self._minhash: Dict[str, Tuple[np.ndarray, int]] = {}  # name -> (MinHash sketch, ACGT bases): write_genome_dist
        self._completed: List[str] = []  # anchor genomes whose files this process completed (Genome._write_tables)

    def _reopen_prepared(self):
        self.prefix = self.input
        if not all(os.path.isfile(f) for f in (self.config_fname, self.samples_fname)):
            raise ValueError("Index write directory not initialized")
        self.input = self.samples_fname
        self.load_config()

    def _create_from_samples(self):
        self.prefix = self.prefix if self.prefix is not None else os.path.dirname(self.input)
        self.prefix = self.prefix or "."
        os.makedirs(self.prefix, exist_ok=True)
        self.init_config()

    def _open_readonly(self):
        self.prefix = self.input
        self.load_config()

    def _check_geometry(self):
        for nm in ("lowres_step", "max_bin_kbp", "min_bin_count"):
            v = getattr(self, nm)
            if not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError(f"{nm} must be a positive integer, got {v!r}")
        if self.lowres_step == 1:
            raise ValueError("lowres_step=1 would name the low-resolution bitmap like the full one (bitmap.1)")

    @property
    def result_geometry(self) -> dict:
        """what every AnchorResult of this index is created with (index.py:101-106, 1169-1172)"""
        return dict(lowres_step=int(self.lowres_step), max_bin_len=int(self.max_bin_kbp) * 1000,
                    min_bin_count=int(self.min_bin_count))

    def _load_samples(self):
        self.samples = pd.read_table(self.samples_fname)
        missing = {"name", "id"} - set(self.samples.columns)
        if missing:
            raise ValueError(f"{self.samples_fname} is missing required column(s): {', '.join(sorted(missing))}. "
                             "This directory does not look like a prepared Panagram index.")
        self.samples = self.samples.set_index("name")
        self.ngenomes = len(self.samples)
        self.genomes: Dict[str, Genome] = {
            name: Genome(self, int(row["id"]), name, row["fasta"], row.get("gff"), bool(row["anchor"]), write=self.write_mode)
            for name, row in self.samples.iterrows()}
        if self.anchor_genomes is None:
            self.anchor_genomes = [n for n, g in self.genomes.items() if g.anchored]

    # ---- naming (index.py:155-165, 359-405) ----
    @property
    def params(self):
        return {k_: v for k_, v in dataclasses.asdict(self).items() if k_ not in self._EXTRA}

    @property
    def config_fname(self):
        return os.path.join(self.prefix, "config.yaml")

    @property
    def samples_fname(self):
        return os.path.join(self.prefix, "samples.tsv")

    @property
    def genome_dist_fname(self):
        return os.path.join(self.prefix, "genome_dist.tsv")

    @property
    def kmer_shared_fname(self):
        return os.path.join(self.prefix, "kmer_shared.tsv")

    @property
    def kmer_occupancy_fname(self):
        return os.path.join(self.prefix, "kmer_occupancy.tsv")

    def get_subdir(self, name):
        return os.path.join(self.prefix, name)

    def kmc_prefix(self, *names):
        return os.path.join(self.get_subdir("kmc"), ".".join(names))

    @property
    def genome_names(self):
        return self.samples.index

    @property
    def kmc_bitvec_count(self):
        return (len(self.samples) + 31) // 32

    @property
    def bitvec_prefixes(self):
        return [self.kmc_prefix(f"bitvec{i}") for i in range(self.kmc_bitvec_count)]

    @property
    def opdef_filenames(self):
        return [self.kmc_prefix(f"opdef{i}.txt") for i in range(self.kmc_bitvec_count)]

    def write_opdefs(self):
        """The `kmc_tools complex` operation files of the reference workflow (index.py:407-426, rule `opdefs`
        workflow/Snakefile:71-79): per 32-sample group, its samples' one-hot databases as inputs and
        ``bitvec{i} = s0 + s1 + ... -ocsum`` as output.  The GPU table build needs none of this; the files are written
        next to the exported ``bitvec{i}`` databases (``--export_kmc``) for a user who keeps `kmc_tools` in the loop."""
        names = [str(n) for n in self.samples.index]
        os.makedirs(self.get_subdir("kmc"), exist_ok=True)
        for i, fname in enumerate(self.opdef_filenames):
            group = names[32 * i:32 * (i + 1)]
            text = ["INPUT:"] + [f"{n} = {self.kmc_prefix(n, 'onehot')}" for n in group]
            text += ["OUTPUT:", f"{self.kmc_prefix(f'bitvec{i}')} = " + " + ".join(group), "-ocsum"]
            with open(fname, "w") as f:
                f.write("\n".join(text) + "\n")

    @property
    def steps(self):
        return (1, self.lowres_step)

    def __getitem__(self, genome):
        return self.genomes[genome]

    # ---- config files (index.py:269-295, 347-357) ----
    @staticmethod
    def _write_atomically(path: str, write) -> None:
        """several ranks of one multi-GPU job write the same bytes: write-then-rename keeps readers whole"""
        tmp = f"{path}.{os.getpid()}.tmp"
        write(tmp)
        os.replace(tmp, path)

    @staticmethod
    def normalise_samples(table: pd.DataFrame, anchor_genomes=None, first_id: int = 0):
        """A user's samples table -> (the schema samples.tsv is stored in — index ``name``; columns fasta, gff, id, anchor —
        and the anchor genomes).  ``anchor_genomes`` None: the table's own anchor column, else every sample with a FASTA.
        Ids count from ``first_id`` (``add``: they continue from the index's)."""
        if not {"name", "fasta"} <= set(table.columns):
            raise ValueError("Input samples must contain 'name' and 'fasta' column headers")
        bad = [str(n) for n in table["name"] if not re.fullmatch(NAME_REGEX, str(n))]
        if bad:
            raise ValueError("Invalid genome names: '" + "', '".join(bad) + f"'\nMust match r'{NAME_REGEX}'.")
        out = table.reindex(columns=["name", "fasta", "gff"] + (["anchor"] if "anchor" in table else []))
        out = out.set_index("name").dropna(how="all")
        out["id"] = np.arange(len(out), dtype=int) + int(first_id)
        if anchor_genomes is None:
            chosen = out["anchor"].astype(bool) if "anchor" in out else out["fasta"].notna()
            anchor_genomes = list(out.index[chosen])
        out["anchor"] = out.index.isin(anchor_genomes)
        return out[list(Index.SAMPLE_COLUMNS)], anchor_genomes

    def _normalised_samples(self, table: pd.DataFrame) -> pd.DataFrame:
        out, self.anchor_genomes = self.normalise_samples(table, self.anchor_genomes)
        return out

    def init_config(self):
        samples = self._normalised_samples(pd.read_table(self.input))
        self._write_atomically(self.samples_fname, lambda tmp: samples.to_csv(tmp, sep="\t"))
        self.write_config()

    def write_config(self, exclude=("prefix",)):
        prms = {k_: v for k_, v in self.params.items() if k_ not in exclude}

        def dump(tmp):
            with open(tmp, "w") as f:
                yaml.dump(prms, f)
        self._write_atomically(self.config_fname, dump)

    def load_config(self):
        with open(self.config_fname) as f:
            stored = yaml.load(f, yaml.SafeLoader) or {}
        for key, val in stored.items():
            if key in self._NOT_IN_CONFIG:
                continue
            section = getattr(self, key, None)
            if dataclasses.is_dataclass(section) and isinstance(val, dict):
                for sub, v in val.items():  # nested sections (kmc, genome_umap, chrom_umap) are updated in place
                    setattr(section, sub, v)
            else:
                setattr(self, key, val)

    # ---- the table: replaces rules kmc_count / opdefs / kmc_bitvec (workflow/Snakefile:54-110) ----
    @property
    def context(self) -> engine.Context:
        if self._ctx is None:
            self._ctx = engine.Context(self.device)
        return self._ctx

    def _pinned_reader_pool(self, names, count: int):
        """a ``_PinnedPool`` for reading the plain FASTA files of ``names`` — buffers as large as the largest of them, at most
        ``count`` and 8 GB in all — or None: less than 256 MB to read that way, or an engine without page-locked buffers (the CPU
        tests' stand-in); the files are then read into pageable arrays"""
        sizes = [os.path.getsize(self.genomes[n].fasta) for n in names if not self.genomes[n].fasta.endswith((".gz", ".bgz"))]
        make = getattr(self.context, "host_buffer", None)
        if not sizes or make is None or os.environ.get("PG_PINNED_READS", "1") in ("0", ""):
            return None
        # (a small job gains nothing: locking and unlocking the pool's memory costs 40 ms per GB each way; PG_PINNED_READS=2: any size)
        if sum(sizes) < (256 << 20) and os.environ.get("PG_PINNED_READS", "1") != "2":
            return None
        cap = max(sizes) + 1  # (+ 1: a file that grew is noticed)
        if cap > (4 << 30):
            return None
        # (four buffers keep the upload busy — a reader fills one in 10-20 ms, the parser empties one in 5-7 — and cost half of what
        # eight cost to lock and unlock: 8 x 100 Mb 0.43 -> 0.39 s, 64 x 200 Mb 2.1-2.2 -> 1.9-2.0 s, tools/e2e_fresh.py)
        count = int(os.environ.get("PG_PINNED_BUFFERS", "0")) or min(count, 4)
        return _PinnedPool(make, cap, max(2, min(count, len(sizes), (8 << 30) // cap)))

    def load_inputs(self):
        """Every sample's sequence parsed and packed on the GPU (0.375 byte per base), with the HyperLogLog
        registers of its distinct canonical k-mers.  Returns ``[(name, genome, seqset, min_count, registers)]`` in
        sample order.  Sketches merge by register-wise maximum, so the distinct k-mers of any union of samples —
        the whole pangenome, or one block of genomes — can be estimated before a table is allocated."""
        if getattr(self, "_inputs", None) is not None:
            return self._inputs
        import time
        from concurrent.futures import ThreadPoolExecutor
        t_start = time.perf_counter()
        inputs = []
        sketch = engine.KmerSketch(self.context, self.k)
        # genome_dist.tsv: each sample's MinHash sketch while its sequence is resident (only the writing rank needs them)
        minhash = engine.MinHashSketch(self.context) if self.genome_dist and self.rank == 0 else None
        # the FASTA files are read a few ahead by host threads while the GPU parses and sketches — plain files straight into a
        # small pool of page-locked buffers (engine.HostBuffer) that go round: the text then goes up by DMA instead of through
        # the runtime's staging copy of pageable memory, and a file costs neither 50 000 page faults nor their unmapping
        # (64 x 200 Mb: 22 -> 10 ms per file beside the readers, tools/attic/r6_load_inputs_breakdown.py)
        todo = [n for n, g in self.genomes.items() if not pd.isna(g.fasta) and not is_fastq(g.fasta) and n not in self._seqsets]
        nread = int(os.environ.get("PG_READERS", "0")) or max(2, min(6, engine.usable_cpus() // 2))
        reader = ThreadPoolExecutor(max_workers=nread)
        pool = self._pinned_reader_pool(todo, nread + 2)
        read = (lambda path: _read_fasta_pinned(path, pool)) if pool is not None else (lambda path: (_read_fasta_image(path), None))
        # (never more files in flight than buffers: a reader that waited for one held by a LATER file's finished read would wait for ever)
        window = pool.budget if pool is not None else nread + 2
        ahead = {n: reader.submit(read, self.genomes[n].fasta) for n in todo[:window]}
        nxt = window
        for name, g in self.genomes.items():
            if pd.isna(g.fasta):
                continue
            if name in ahead:
                t0 = time.perf_counter()
                image, buf = ahead.pop(name).result()
                t1 = time.perf_counter()
                self._seqsets[name] = engine.SeqSet.from_fasta(self.context, image)
                del image
                if buf is not None:
                    pool.put(buf)  # (the text is on the device: the buffer takes the next file)
                # (where a load's time goes: waiting for the readers / upload + parse + pack of the text)
                self.timings["load_wait_read_s"] = self.timings.get("load_wait_read_s", 0.0) + t1 - t0
                self.timings["load_parse_s"] = self.timings.get("load_parse_s", 0.0) + time.perf_counter() - t1
                if nxt < len(todo):
                    ahead[todo[nxt]] = reader.submit(read, self.genomes[todo[nxt]].fasta)
                    nxt += 1
            if is_fastq(g.fasta):
                # read sets: kmc -ci2 -fq (workflow/Snakefile:88-89) — k-mers seen once are dropped
                # (the sketch counts them too: the table is sized from above)
                if name in self.anchor_genomes:
                    raise ValueError(f"{name}: a FASTQ sample cannot be an anchor genome")
                ss, min_count = engine.SeqSet.from_host(self.context, [read_fastq_joined(g.fasta)]), 2
            else:
                ss, min_count = self.seqset_for(name), 1
            t0 = time.perf_counter()
            sketch.reset()
            sketch.add(ss)
            inputs.append((name, g, ss, min_count, sketch.registers()))
            self.timings["load_sketch_s"] = self.timings.get("load_sketch_s", 0.0) + time.perf_counter() - t0
            if minhash is not None and name not in self._minhash:
                t0 = time.perf_counter()
                self._minhash[name] = self._minhash_of(minhash, ss, engine.KmerSketch.estimate_registers(inputs[-1][4]))
                self.timings["load_minhash_s"] = self.timings.get("load_minhash_s", 0.0) + time.perf_counter() - t0
        if pool is not None:
            reader.submit(pool.close)  # (unlocking the memory costs as much as locking it, 40 ms per GB: beside the table build)
        reader.shutdown(wait=False)
        sketch.close()
        if minhash is not None:
            minhash.close()
        self.context.trim()  # (the FASTA text buffer the parser kept for the next file)
        self._inputs = inputs
        self.timings["load_inputs_s"] = self.timings.get("load_inputs_s", 0.0) + time.perf_counter() - t_start
        return inputs

    @staticmethod
    def _expected_keys(inputs) -> int:
        """distinct canonical k-mers of the union of ``inputs`` (+3 %: the sketch's standard error is 0.4 %)"""
        if not inputs:
            return 1024
        regs = np.maximum.reduce([i[4] for i in inputs])
        est = engine.KmerSketch.estimate_registers(regs)
        return est + est // 32 + 1024

    def _replicated_keys(self, inputs) -> int:
        """distinct k-mers of the largest table a rank holds in the replicated mode: the union of the genomes it anchors
        (``build_table``'s filtered build) — or of all samples where that build does not apply.  The same answer in
        every process."""
        if not (self.filtered_table and not self.export_kmc and not self.kmer_stats and all(i[3] <= 1 for i in inputs)):
            return self._expected_keys(inputs)
        if self.world > 1 and os.environ.get("PG_PARTITION", "pieces") != "genomes":
            # pieces of homology classes: a rank's table is built from its 1 / world of the anchored sequence
            # (+30 %: the pieces are only balanced to a piece, and k-mers of repeats occur in several ranks' shares)
            return int(self._expected_keys([i for i in inputs if i[0] in self.anchor_genomes]) * 1.3 / self.world) + 1024
        writer = self.writer_of_anchor() if self.world > 1 else {a: 0 for a in self.anchor_genomes}
        worst = 0
        for r in range(max(1, self.world)):
            mine = [i for i in inputs if writer.get(i[0]) == r]
            worst = max(worst, self._expected_keys(mine) if mine else 0)
        return worst or self._expected_keys(inputs)

    def _roomy_density(self, expected_keys: int, anchors, inputs=None) -> float:
        """keys per 128-byte line for the table about to be built (0: the library's 3): sparser where HBM is plentiful — it has to
        leave room for two batches of rows (one being written, one being anchored: ``batch_bytes`` each at most) of the
        anchors given (names, or {name: SeqSet} of pieces) — and the genomes are not repeat-rich (the longest input's sketch:
        distinct k-mers per position).  engine.PanTable.roomy_density."""
        nb = (self.ngenomes + 7) // 8
        if isinstance(anchors, dict):
            rows = sum(int(ss.lens.sum()) for ss in anchors.values()) * nb
        else:
            rows = sum(os.path.getsize(self.genomes[n].fasta) for n in anchors if n in self.genomes) * nb  # (a byte of FASTA per position, about)
        distinct = None
        if inputs:
            big = max(inputs, key=lambda i: int(i[2].lens.sum()))
            npos = max(1, int(big[2].lens.sum()))
            distinct = min(1.0, engine.KmerSketch.estimate_registers(big[4]) / npos)
        return engine.PanTable.roomy_density(self.context, self.k, self.ngenomes, expected_keys, 2 * min(self.batch_bytes, rows) + rows // 50,
                                             distinct_fraction=distinct)

    def build_table(self, keep: Optional[Sequence[str]] = None, insert_sets: Optional[Dict[str, "engine.SeqSet"]] = None) -> engine.PanTable:
        """``keep``: the genomes whose packed sequences stay resident for the anchor step (default: all anchors) — and,
        in the filtered build, the genomes whose k-mers the table is built from.  ``insert_sets`` (the contig-sharded
        multi-GPU mode): ``{genome: SeqSet}`` of the PIECES this process anchors — the table is built from those pieces,
        every sample then only sets its bits."""
        keep = set(self.anchor_genomes if keep is None else keep)
        if self._table is not None:
            # a filtered table answers only for what it was built from: anything else would silently read as absent
            scope = self._table_scope
            if scope != "all" and (insert_sets is not None or scope == "pieces" or not keep <= scope):
                raise RuntimeError("the cached table was built for " + ("this process's pieces" if scope == "pieces" else f"the anchors {sorted(scope)}") +
                                   " only; close() the index before building a table for other anchors")
            return self._table
        have = all(os.path.exists(p + ".kmc_pre") and os.path.exists(p + ".kmc_suf") for p in self.bitvec_prefixes)
        scope = "all"
        import time
        t_start, t_inputs_before = time.perf_counter(), self.timings.get("load_inputs_s", 0.0)
        # how the table will be probed decides its minimizer window with the key count (pg_table_set_coscheduled): the anchor
        # genomes of a batch share ONE co-scheduled launch; a single anchor has no partner
        cosched = max(1, len(keep if insert_sets is None else insert_sets))
        if self.kmc.use_existing and have:
            tbl = engine.PanTable(self.context, self.k, self.ngenomes, coscheduled=cosched)
            for i, p in enumerate(self.bitvec_prefixes):
                tbl.load_kmc_files(i, p)
            logger.info("KMC Database Loaded")
        else:
            # every input is parsed and packed once on the GPU (0.375 byte per base) and stays
            # resident through the build; a sketch of the distinct k-mers over all of them sizes the
            # table (and settles its minimizer length) once: no re-hash while it grows, no second
            # copy of the table in HBM.  Anchors keep their sequences for the anchor step.
            inputs = self.load_inputs()
            # The anchor step only ever asks for k-mers of the sequence THIS process anchors (``keep`` genomes, or the
            # pieces in ``insert_sets``): the table is built from that and the other samples only set their bits in it
            # (pg_table_update_seqset) — the rows are the ones the table of all genomes gives, the table is as small as
            # the anchored sequence's own k-mer set (a rank of a multi-GPU run, or a pangenome in which only some genomes
            # are anchors).  Not when the merged databases are to be exported, nor with read-set samples (their -ci2
            # count tables merge through the inserting path), nor when the pan-genome's k-mer statistics are wanted (kmer_stats:
            # they describe the k-mers the table was built from).
            first = [i for i in inputs if i[0] in keep]
            rest = [i for i in inputs if i[0] not in keep]
            can_filter = self.filtered_table and not self.export_kmc and not self.kmer_stats and all(i[3] <= 1 for i in inputs)
            if insert_sets is not None and can_filter:
                sketch = engine.KmerSketch(self.context, self.k)
                for ss in insert_sets.values():
                    sketch.add(ss)
                est = sketch.estimate()
                sketch.close()
                expected = est + est // 32 + 1024
                tbl = engine.PanTable(self.context, self.k, self.ngenomes, expected_keys=expected, coscheduled=cosched,
                                      keys_per_line=self._roomy_density(expected, keep if insert_sets is None else insert_sets, inputs))
                for name, ss in insert_sets.items():
                    tbl.insert_seqset(self.genomes[name].id, ss)
                for name, g, ss, _, _ in inputs:
                    tbl.update_seqset(g.id, ss)
                    if name not in keep:
                        self.drop_seqset(name)
                scope, filtered = "pieces", True
            else:
                filtered = bool(can_filter and first and rest)
                expected = self._expected_keys(first if filtered else inputs)
                tbl = engine.PanTable(self.context, self.k, self.ngenomes, expected_keys=expected, coscheduled=cosched,
                                      keys_per_line=self._roomy_density(expected, keep, inputs))
                for name, g, ss, min_count, _ in (first + rest if filtered else inputs):
                    if filtered and name not in keep:
                        tbl.update_seqset(g.id, ss)
                    else:
                        tbl.insert_seqset(g.id, ss, min_count=min_count)
                    if min_count > 1:
                        ss.close()
                    elif name not in keep:
                        self.drop_seqset(name)
                if filtered:
                    scope = frozenset(i[0] for i in first)
            self._inputs = None
            logger.info("k-mer table built on GPU (sketch: %d distinct k-mers%s): %s", expected,
                        (" of this process's pieces" if scope == "pieces" else f" of the {len(first)} genomes anchored here") if filtered else "",
                        tbl.stats())
            if self.export_kmc:
                os.makedirs(self.get_subdir("kmc"), exist_ok=True)
                for i, p in enumerate(self.bitvec_prefixes):
                    keys, vals = tbl.export(i)
                    write_kmc1(p, keys, vals, self.k)
                self.write_opdefs()
        self.context.synchronize()
        # (the inserts alone: reading, parsing and sketching the inputs is load_inputs_s, also when it ran in here)
        self.timings["table_build_s"] = time.perf_counter() - t_start - (self.timings.get("load_inputs_s", 0.0) - t_inputs_before)
        self._table, self._table_scope = tbl, scope
        return tbl

    # ---- genome_dist.tsv: rule `mash` of the reference workflow (workflow/Snakefile:124-149) ----
    @staticmethod
    def _minhash_of(minhash: "engine.MinHashSketch", ss: "engine.SeqSet", distinct: int = 0) -> Tuple[np.ndarray, int]:
        minhash.reset()
        minhash.add(ss, distinct)
        return minhash.result()

    def write_genome_dist(self, exact: bool = False) -> str:
        """Write ``genome_dist.tsv`` — what the reference's workflow makes with ``mash sketch -r -s 10000`` and ``mash
        triangle -E`` (workflow/Snakefile:124-149) and ``panagram view`` reads at start-up (figs.py:50-59): one line per
        pair of samples in sample order, ``name_a, name_b, distance, p-value, common/denom``, numbers as %.6g.

        The sketches (engine.MinHashSketch: the 10 000 smallest MurmurHash3 values of the canonical 21-mers, seed 42, mash's
        defaults whatever this index's k) come from ``load_inputs`` when ``genome_dist`` was set; the samples without one
        are read, sketched and freed one at a time.  Distances: mash's merge and formula (engine.minhash_distances).  The
        p-value uses each sample's ACGT bases where mash under ``-r`` estimates a genome size, so that column can differ
        from mash's; the viewer reads only the names and the distance.  Byte-for-byte agreement with mash 2.3 is the intent,
        not a tested claim.  Returns the file's path.

        ``exact``: the same file from the pan table's shared distinct k-mer counts (``kmer_stats``) in place of sketches —
        same five columns, same pair order, numbers as %.6g: the distance is mash's formula on the EXACT Jaccard index at
        this index's k (not an estimate at k = 21), the p-value column the literal ``0`` (nothing was sampled), the last
        column ``shared/union`` in distinct k-mers.  The default writes what it always wrote."""
        names = [str(n) for n in self.genome_names]
        if exact:
            from . import pangenome
            lines = pangenome.genome_dist_lines(names, self._kmer_stats_raw()["pairs"], self.k)

            def write_exact(tmp):
                with open(tmp, "w") as f:
                    f.write("".join(lines))
            self._write_atomically(self.genome_dist_fname, write_exact)
            return self.genome_dist_fname
        todo = [n for n in names if n not in self._minhash]
        if todo:
            minhash = engine.MinHashSketch(self.context)
            hll = engine.KmerSketch(self.context, engine.MinHashSketch.K)
            try:
                for name in todo:
                    g = self.genomes[name]
                    if pd.isna(g.fasta):
                        self._minhash[name] = (np.zeros(0, np.uint64), 0)
                        continue
                    resident = self._seqsets.get(name)
                    if resident is not None:
                        ss = resident
                    elif is_fastq(g.fasta):
                        ss = engine.SeqSet.from_host(self.context, [read_fastq_joined(g.fasta)])
                    else:
                        ss = engine.SeqSet.from_fasta(self.context, g.fasta)
                    hll.reset()
                    hll.add(ss)
                    self._minhash[name] = self._minhash_of(minhash, ss, hll.estimate())
                    if ss is not resident:
                        ss.close()
            finally:
                hll.close()
                minhash.close()
        sketches = [self._minhash[n][0] for n in names]
        bases = [self._minhash[n][1] for n in names]
        dist, pval, common, denom = engine.minhash_distances(sketches, bases)
        lines, t = [], 0
        for i in range(len(names)):
            for j in range(i + 1, len(names)):
                lines.append(f"{names[i]}\t{names[j]}\t{dist[t]:.6g}\t{pval[t]:.6g}\t{common[t]}/{denom[t]}\n")
                t += 1

        def write(tmp):
            with open(tmp, "w") as f:
                f.write("".join(lines))
        self._write_atomically(self.genome_dist_fname, write)
        return self.genome_dist_fname

    # ---- the pan-genome's own k-mer statistics (pangenome.py), off the pan table ----
    def _full_table(self) -> engine.PanTable:
        """the table of EVERY sample's k-mers: the cached one when it is that, else built now with filtering off and cached"""
        if self._table is not None:
            scope = self._table_scope
            if scope != "all":
                raise RuntimeError("the cached table was built for " + ("this process's pieces" if scope == "pieces" else f"the anchors {sorted(scope)}") +
                                   " only; close() the index before building a table for other anchors")
            return self._table
        filtered, self.filtered_table = self.filtered_table, False
        try:
            return self.build_table()
        finally:
            self.filtered_table = filtered

    def _kmer_stats_raw(self) -> dict:
        return self._full_table().kmer_stats()

    def _kmer_stats_frames(self):
        """``kmer_stats()``: (shared, genomes) — the shared distinct k-mers of every pair of samples as a named matrix, and per
        sample its distinct, private, core and shell k-mers (pangenome.frames) — counted on the GPU in one pass over the
        table of all samples' k-mers.  A cached table that was built from some anchors' k-mers only cannot answer: RuntimeError."""
        from . import pangenome
        return pangenome.frames(self._kmer_stats_raw(), self.genome_names)

    def write_kmer_stats(self) -> Tuple[str, str]:
        """Write ``kmer_shared.tsv`` (the shared-k-mer matrix: a header row, a ``name`` column) and ``kmer_occupancy.tsv``
        (columns ``n``, ``kmers``: distinct k-mers held by exactly n samples) into the index directory; returns their paths."""
        from . import pangenome
        stats = self._kmer_stats_raw()
        shared, _ = pangenome.frames(stats, self.genome_names)
        occ = pangenome.occupancy_frame(stats)
        self._write_atomically(self.kmer_shared_fname, lambda tmp: shared.to_csv(tmp, sep="\t", index_label="name"))
        self._write_atomically(self.kmer_occupancy_fname, lambda tmp: occ.to_csv(tmp, sep="\t", index=False))
        return self.kmer_shared_fname, self.kmer_occupancy_fname

    def seqset_for(self, name: str) -> engine.SeqSet:
        """The genome's FASTA, parsed and 2-bit packed in HBM (0.375 byte per base), cached."""
        ss = self._seqsets.get(name)
        if ss is None:
            ss = self._seqsets[name] = engine.SeqSet.from_fasta(self.context, self.genomes[name].fasta)
        return ss

    def drop_seqset(self, name: str) -> None:
        ss = self._seqsets.pop(name, None)
        if ss is not None:
            ss.close()

    # ---- which multi-GPU mode ----
    HBM_RESERVE = 8 << 30  # left alone next to the table: packed sequences, descriptors, the writers' staging

    def plan_sharding(self):
        """("replicated", 1) — one table of all genomes on every GPU, anchor genomes dealt to the ranks, no
        collective — or ("genome", nblocks): the pangenome's tables do not fit one GPU next to a working set of
        rows, so the genomes are cut into ``nblocks`` contiguous blocks, a GPU holds the table of ONE block at a
        time, every GPU probes every anchor position against its block and the blocks' bit columns are
        all-gathered (``distributed.run_genome_sharded``).  ``nblocks`` is the smallest multiple of the world
        size whose largest block fits; more blocks than GPUs run as passes.  ``shard`` / ``genome_blocks``
        (``PG_SHARD``, ``PG_GENOME_BLOCKS``) override the choice."""
        if self.shard not in (None, "replicated", "genome"):
            raise ValueError(f"shard must be 'replicated' or 'genome', got {self.shard!r}")
        if self.shard == "replicated":
            return "replicated", 1
        have = all(os.path.exists(p + ".kmc_pre") and os.path.exists(p + ".kmc_suf") for p in self.bitvec_prefixes)
        if self.kmc.use_existing and have and self.shard is None:
            return "replicated", 1  # merged bitvec databases cannot be cut into genome blocks
        N = self.ngenomes
        if self.shard == "genome" and self.genome_blocks > 0:
            return "genome", min(N, self.genome_blocks)
        inputs = self.load_inputs()
        free = self._agreed_free_memory()
        nb = (N + 7) // 8
        longest = max([int(i[2].lens.sum()) for i in inputs if i[0] in self.anchor_genomes] or [0])
        # next to the table: two batches of rows (one being written, one being anchored), at least one anchor each
        budget = free - self.HBM_RESERVE - 2 * min(self.batch_bytes, max(longest * nb, 1 << 30))
        by_id = {i[1].id: i for i in inputs}
        if self.shard is None and engine.PanTable.bytes_for(self.k, N, self._replicated_keys(inputs)) <= budget:
            return "replicated", 1
        # Candidates: nblocks = world, 2 world, ... — FEWER blocks mean fewer passes over the anchors' positions, and a block
        # table may be created DENSER than the library's 3 keys per line to make its genomes' union fit (round 6,
        # pg_table_create_dense): a pass against a denser, wider block is slower (``_block_rate``, measured on BASELINE
        # configs[4]: 8 x 3 Gb at d = 0.05 on one GPU — two genomes per block at 3.4-3.6 keys per line take 4 passes of 0.27 s
        # where one genome per block took 8 of 0.21 s: 14.1 -> 23 G k-mers/s for the job), so the cheapest candidate by
        # passes / rate wins; the search ends at the first candidate that fits at the library's density — more blocks only
        # add passes from there.
        anchor_positions = sum(int(i[2].lens.sum()) for i in inputs if i[0] in self.anchor_genomes)
        best = None  # (cost, nblocks, keys_per_line)
        nblocks = max(1, self.world)
        while True:
            nblocks = min(nblocks, N)
            per = (N + nblocks - 1) // nblocks
            keys = 0
            for b0 in range(0, N, per):
                blk = [by_id[g] for g in range(b0, min(N, b0 + per)) if g in by_id]
                keys = max(keys, self._expected_keys(blk))
            worst = engine.PanTable.bytes_for(self.k, per, keys)
            # a block's table sits next to the anchors' rows of ITS genomes only (ceil(per/8) bytes per anchor position, every
            # anchor's: each rank probes them all — unless the probe emits the block's columns directly) and the full-width
            # rows this rank holds as a writer: with several passes those of ALL its anchors (they gather bits pass by
            # pass), with one pass those whose writer jobs are still in flight (run_genome_sharded bounds them)
            mine = -(-len(self.anchor_genomes) // max(1, self.world))
            passes = -(-((N + per - 1) // per) // max(1, self.world))
            resident = (mine if passes > 1 else min(mine, 2 * self.writer_jobs(longest * nb * mine) + 1)) * longest * nb
            avail = free - self.HBM_RESERVE - max(2 * longest * nb, resident)
            fits_sparse = worst <= avail
            if fits_sparse:
                cand = (passes / self._block_rate(per, 3.0), (N + per - 1) // per, 0.0, False)
            else:
                # (blocks of one or two genomes that only fit dense have the probe emit their bit columns itself — no narrow
                # rows, one byte per anchor position more for the table: configs[4] on one GPU 3.6 -> 3.2 keys per line, +5 %)
                from .distributed import ShardedAnchoring
                direct = per <= 2 or (engine.COLUMNS_DIRECT and per <= min(8, ShardedAnchoring.DIRECT_MAX_WIDTH))
                room = avail - (0 if direct else anchor_positions * ((per + 7) // 8))
                kpl = keys * 128.0 * 1.02 / room if room > 0 else float("inf")  # (+2 %: the line count is rounded up to a prime)
                kpl = max(kpl, 3.05)
                cand = (passes / self._block_rate(per, kpl), (N + per - 1) // per, round(kpl + 0.05, 1), direct and per <= 2) if (per <= 64 and kpl <= self.BLOCK_KPL_MAX) else None
            if cand is not None and (best is None or cand[0] < best[0] - 1e-9):
                best = cand
            if fits_sparse or nblocks >= N:
                if best is None:  # (nothing fits by this arithmetic: one genome per block at the library's density, as before)
                    best = (0.0, (N + per - 1) // per, 0.0, False)
                self._block_keys_per_line, self._block_direct = best[2], best[3]
                return "genome", best[1]
            nblocks += max(1, self.world)

    # relative probe rate of a pass against a block table of ``per`` genomes at ``kpl`` keys per 128-byte line (8 x 3 Gb, d = 0.05,
    # one MI355X; profiles/r6g*_config5_blocks.txt): G k-mers/s per pass 112 at (1, 3.0); (2, .): 94 at 3.2, 93 at 3.4, 90 at 3.6,
    # 86-89 at 4.0, 80 at 4.5, 61 at 5.5, 45 at 6.2; 45 at (4, 5.8)
    BLOCK_KPL = ((3.0, 1.0), (3.6, 0.955), (4.0, 0.92), (4.5, 0.845), (5.5, 0.65), (6.2, 0.476))
    BLOCK_KPL_MAX = 6.2
    _block_keys_per_line = 0.0  # what plan_sharding chose for the block tables (0: the library's density)
    _block_direct = False       # ... and whether the probe emits the blocks' bit columns itself (no narrow rows)

    @classmethod
    def _block_rate(cls, per: int, kpl: float) -> float:
        pts = cls.BLOCK_KPL
        if kpl <= pts[0][0]:
            r = pts[0][1]
        elif kpl >= pts[-1][0]:
            r = pts[-1][1]
        else:
            r = next(a[1] + (b[1] - a[1]) * (kpl - a[0]) / (b[0] - a[0]) for a, b in zip(pts, pts[1:]) if a[0] <= kpl <= b[0])
        return r * max(1, per) ** -0.27

    # ---- panagram index command (index.py:172-191) ----
    def run(self):
        """Table build, then the anchors in batches: the anchor genomes of a batch share ONE
        co-scheduled launch (homologous regions side by side, table lines shared in L2 — the
        reference runs one thread per anchor FASTA instead, cpp/anchor.cpp:217-223), and host threads
        stream each genome's rows out of HBM into its BGZF files while the next batch is anchored.
        A pangenome whose table does not fit one GPU goes through the genome-sharded mode instead
        (``plan_sharding``)."""
        if self.kmer_stats and self.world > 1:
            # (a rank's table holds its pieces' or its genome block's k-mers, never the pan-genome's)
            raise ValueError("kmer_stats needs the one table of all samples' k-mers: it is single-GPU, and this run has "
                             f"{self.world} processes")
        print("Wrote config.yaml and samples.tsv")
        if self.prepare:
            print("Prepared. Run 'python -m panagram_amd index <dir>' to build the index")
            return
        from concurrent.futures import ThreadPoolExecutor
        import time
        self._run_t0, self._cpu_t0 = time.perf_counter(), time.process_time()
        os.makedirs(self.get_subdir("logs"), exist_ok=True)
        own_group = self._ensure_process_group()
        try:
            self._run_planned(ThreadPoolExecutor)
            if self.annotate:  # (every mode: the process that completed a genome's files annotates it)
                for name in list(self._completed):
                    if self.genomes[name].annotated:
                        self.genomes[name].run_annotate()
                self.close()
            if self.umaps:  # (as above: by the process that completed the genome's files)
                for name in list(self._completed):
                    self.genomes[name].write_umaps()
                self.close()
            if self.genome_dist and self.rank == 0:  # (one writer in a multi-rank run)
                self.write_genome_dist()
                self.close()
        finally:
            if own_group:
                self._dist().destroy_process_group()

    add_breakdown = False  # ``add``: also time probe / inflate / append / statistics into ``timings`` (a device synchronise after each)

    def add(self, new_samples) -> List[str]:
        """Append samples to this finished index without re-anchoring it (add.py; no reference counterpart).  ``new_samples``:
        a table (path or DataFrame) in the input schema of ``samples.tsv`` — name, fasta, optional gff and anchor — listing the
        NEW samples only; ids continue from this index's.  Every anchor already in the index gets its rows widened by the new
        samples' columns (its FASTA probed against the new samples' k-mers alone, its old rows read back from bitmap.1.gz, one
        kernel pass: ``AnchorResult.append_columns``) and all of its files rewritten by the code that writes them in ``run``;
        new anchors are anchored the ordinary way.  Everything is staged inside the index and renamed at the end, samples.tsv
        last.  Refused before any file is touched (ValueError): a name already in the index, a missing FASTA, an old anchor
        without bitmap.1.gz or chrs.tsv, more than one process, a read-only index.  Returns one line per anchor rewritten and
        per anchor added.  Afterwards this object describes all N + m samples and is left as ``run`` leaves it: ``close()``d —
        table, packed sequences and GPU context freed; a later call makes a context again."""
        from . import add as _add
        return _add.add(self, new_samples)

    def subset(self, out_dir, keep=None, drop=None, anchors=None, sequence_files: bool = True) -> List[str]:
        """Write an index of chosen samples of this finished index into the new directory ``out_dir`` (subset.py; no reference
        counterpart).  ``keep``: the samples to keep, in the order given (``"A,B"`` or a sequence: this is how columns are
        reordered); or ``drop``: the samples to leave out, the rest keeping the index's order.  Ids are renumbered.  Every kept
        anchor (``anchors``: only these of them) gets its rows read back from bitmap.1.gz and narrowed in one kernel pass
        (``AnchorResult.select_columns``), and all of its files written by the code that writes them in ``run``: the tree equals
        ``run`` over the kept samples.  No FASTA is read — unless this index holds kmc/bitvec*, genome_dist.tsv or the k-mer
        statistics, which are refreshed from the kept samples' sequences (``sequence_files=False``: left out instead).  This
        index is never touched (read-only is enough).  Refused before ``out_dir`` is created (ValueError): an unknown or repeated
        name, both or neither of ``keep`` and ``drop``, nothing kept, ``anchors`` naming no kept anchor, a non-empty ``out_dir``
        or one inside this index, a kept anchor without bitmap.1.gz, .gzi or chrs.tsv, more than one process.  A failure midway
        removes ``out_dir``.  Returns one line per anchor of this index, rewritten or left behind; afterwards this object is
        ``close()``d, as ``add`` leaves it."""
        from . import subset as _subset
        return _subset.subset(self, out_dir, keep, drop, anchors, sequence_files)

    def _ensure_process_group(self) -> bool:
        """Under a launcher that set up a rendezvous (torchrun: MASTER_ADDR / MASTER_PORT, RANK, WORLD_SIZE) a run with
        several ranks joins the process group itself — backend "nccl" (= RCCL over xGMI), this rank's GPU — so that the
        ranks can agree on the plan and, in the genome-sharded mode, exchange their bit columns.  Returns whether this
        call created the group (the caller then destroys it).  Without a rendezvous in the environment (ranks run by
        hand, one after the other: the tests) nothing is initialised — the contig-sharded mode needs no group."""
        if self.world <= 1 or "MASTER_ADDR" not in os.environ or int(os.environ.get("WORLD_SIZE", "1")) != self.world:
            return False
        import torch
        import torch.distributed as dist
        if dist.is_initialized():
            return False
        backend = os.environ.get("PG_DIST_BACKEND", "nccl")
        if backend == "nccl":
            torch.cuda.set_device(self.device)
            dist.init_process_group("nccl", rank=self.rank, world_size=self.world, device_id=torch.device("cuda", self.device))
        else:
            dist.init_process_group(backend, rank=self.rank, world_size=self.world)
        return True

    def _run_planned(self, ThreadPoolExecutor):
        import time
        mode, nblocks = self.plan_sharding()
        self._check_plan_agreed((mode, nblocks, self._block_keys_per_line if mode == "genome" else 0.0))
        if mode == "genome":
            if self.kmer_stats:  # (a genome block's table holds its block's bits only)
                raise ValueError("kmer_stats needs the one table of all samples' k-mers, and this pan-genome is indexed in genome blocks")
            from .distributed import run_genome_sharded
            logger.info("genome-sharded mode: %d genome blocks over %d GPU(s)%s", nblocks, self.world,
                        f", block tables at {self._block_keys_per_line:g} keys per line" if self._block_keys_per_line else "")
            self.exchange_stats = {}  # what this rank's exchange moved (bytes_received, passes, chunks): distributed.run_genome_sharded
            run_genome_sharded(self, nblocks, exchange_stats=self.exchange_stats)
            self.close()
            return
        if self.world > 1 and os.environ.get("PG_PARTITION", "pieces") != "genomes":
            # several GPUs, a table that fits one: pieces of homology classes are dealt to the ranks, so that every
            # rank's launch still co-schedules ALL anchor genomes (distributed.run_index_sharded); dealing whole
            # genomes to ranks (PG_PARTITION=genomes, below) leaves a rank's launch without co-scheduling partners —
            # and GPUs idle when there are fewer anchors than GPUs
            from .distributed import run_index_sharded
            run_index_sharded(self, self.rank, self.world, self._barrier())
            self.close()
            return
        mine = self.my_anchor_genomes()
        if not mine:  # more ranks than anchor genomes
            logger.info("rank %d of %d: no anchor genome to write", self.rank, self.world)
            self.close()
            return
        tbl = self.build_table(keep=mine)
        if self.kmer_stats:
            self.write_kmer_stats()
        nb = (self.ngenomes + 7) // 8
        # two batches of rows are resident at a time (one being written, one being anchored), next to the
        # table: with a table that fills most of the HBM the batches shrink to what is left
        free = self.context.mem_info()[0]
        batch_bytes = int(min(self.batch_bytes, max(1 << 30, (free - (6 << 30)) / 2.3)))
        batches, cur, cur_bytes = [], [], 0
        for name in mine:  # a batch's rows stay in HBM until written: bound them
            rows_bytes = int(self.seqset_for(name).lens.sum()) * nb
            if cur and cur_bytes + rows_bytes > batch_bytes:
                batches.append(cur)
                cur, cur_bytes = [], 0
            cur.append(name)
            cur_bytes += rows_bytes
        if cur:
            batches.append(cur)
        # (a writer job is bound by the file system — about 1.5 GB/s of compressed bytes each — not by the GPU;
        # each concurrent job pins its own staging at first use, which only pays for itself on big outputs)
        payload = sum(int(self.seqset_for(n).lens.sum()) for n in mine) * nb
        with ThreadPoolExecutor(max_workers=self.writer_jobs(payload)) as pool:
            previous = None
            for batch in batches:
                t0 = time.perf_counter()
                job = self._anchor_batch(tbl, batch)
                t1 = time.perf_counter()
                futs = [pool.submit(self.genomes[name].write_from_result, job, gi) for gi, name in enumerate(batch)]
                if previous is not None:  # at most two batches of rows resident
                    self._finish_batch(*previous)
                previous = (job, batch, futs)
                # (where the time of a multi-batch run goes: rows allocated + anchored + tabulated / waiting for the writers of the batch before)
                self.timings["anchor_batches_s"] = self.timings.get("anchor_batches_s", 0.0) + t1 - t0
                self.timings["writers_wait_s"] = self.timings.get("writers_wait_s", 0.0) + time.perf_counter() - t1
            t1 = time.perf_counter()
            if previous is not None:
                self._finish_batch(*previous)
            self.timings["writers_wait_s"] = self.timings.get("writers_wait_s", 0.0) + time.perf_counter() - t1
            self.timings["batches"] = len(batches)
        self.close()

    @staticmethod
    def _dist():
        """torch.distributed when this process is part of an initialised process group, else None (torch is not
        imported for a single process)"""
        import sys
        td = sys.modules.get("torch.distributed")
        return td if td is not None and td.is_available() and td.is_initialized() else None

    def _barrier(self):
        d = self._dist()
        return d.barrier if d is not None and self.world > 1 else None

    def _agreed_free_memory(self) -> int:
        """HBM this process may plan with — THE SAME NUMBER ON EVERY RANK, since ranks that decide differently (one
        replicated, one genome-sharded; or different block counts) would meet in mismatched collectives: the minimum of
        the ranks' free memory when a process group exists, else (several ranks without one) the device's total minus
        a fixed allowance for other tenants, else this device's free memory."""
        free, total = self.context.mem_info()
        if self.world <= 1:
            return free
        d = self._dist()
        if d is None:
            return total - (8 << 30)
        import torch
        dev = self.context.torch_device() if d.get_backend() == "nccl" else torch.device("cpu")
        t = torch.tensor([free], dtype=torch.int64, device=dev)
        d.all_reduce(t, op=d.ReduceOp.MIN)
        return int(t.item())

    def _check_plan_agreed(self, plan) -> None:
        """every rank must have reached the same (mode, nblocks) before any of them enters a collective"""
        d = self._dist()
        if d is None or self.world <= 1:
            return
        got = [None] * self.world
        d.all_gather_object(got, (plan[0], int(plan[1])) + tuple(plan[2:]))
        if any(g != got[0] for g in got):
            raise RuntimeError(f"the ranks planned different sharding modes {got}: pin one with PG_SHARD / PG_GENOME_BLOCKS")

    @staticmethod
    def writer_jobs(payload_bytes: int) -> int:
        return int(os.environ.get("PG_WRITERS", "4" if payload_bytes > (4 << 30) else "2"))

    def writer_of_anchor(self) -> Dict[str, int]:
        """anchor genome -> the rank that writes its directory: dealt longest-first (FASTA size), the same answer
        in every process"""
        from .distributed import plan_shards
        units = [(n, 0, os.path.getsize(self.genomes[n].fasta)) for n in self.anchor_genomes]
        return {u[0]: r for r, sh in enumerate(plan_shards(units, max(1, self.world))) for u in sh}

    def my_anchor_genomes(self) -> List[str]:
        """Multi-GPU (one process per GPU, e.g. under torchrun: RANK / WORLD_SIZE): the table is
        replicated — every rank builds it from all inputs — and the anchor GENOMES are dealt to the
        ranks longest-first (FASTA size); each rank writes the directories of its genomes.  Anchors are
        independent (cpp/anchor.cpp:217-223 runs them as OpenMP iterations), so there is no collective
        and the files do not depend on the GPU count."""
        if self.world <= 1:
            return list(self.anchor_genomes)
        w = self.writer_of_anchor()
        return [n for n in self.anchor_genomes if w[n] == self.rank]

    batch_bytes = 32 << 30  # rows of one batch of anchor genomes held in HBM (bitmap.1 payload bytes)
    # BGZF compression of the bitmaps: a zlib level (host threads), or -2 = on the GPU (k_row_deflate)
    bgzf_level = int(os.environ.get("PG_BGZF_LEVEL", "-2"))

    def _anchor_batch(self, tbl, batch):
        sets = [self.seqset_for(name) for name in batch]
        merged = engine.SeqSet.concat(self.context, sets) if len(sets) > 1 else sets[0]
        for name, ss in zip(batch, sets):
            g = self.genomes[name]
            g.ensure_log()
            for nm, ln in zip(ss.names, ss.lens):
                if int(ln) < tbl.k:
                    g.log.warning(f"Contig {nm} is shorter than k={tbl.k}: 0 k-mers (the reference underflows here)")
            g.log.info("Anchoring Started")
        res = engine.AnchorResult(tbl, merged, colsums=True, **self.result_geometry)
        first = np.cumsum([0] + [len(s.names) for s in sets])
        if len(sets) > 1:  # homologous chromosomes side by side, matched by record id whatever order a FASTA lists them in
            res.coschedule(np.repeat(np.arange(len(sets)), [len(s.names) for s in sets]),
                           contig_class=engine.homology_classes([s.names for s in sets]))
        res.run()
        return dict(res=res, merged=merged if len(sets) > 1 else None,
                    genomes=[self.genomes[name].tabulate(res, int(first[gi]), int(first[gi + 1]), list(merged.names[first[gi]:first[gi + 1]]))
                             for gi, name in enumerate(batch)])

    def _finish_batch(self, job, batch, futs):
        try:
            for f in futs:
                f.result()
        finally:
            job["res"].close()
            if job["merged"] is not None:
                job["merged"].close()
            # (the batch's packed sequences — 0.375 byte per base — stay until close(): every hipFree waits
            # for the device, i.e. for the writers' kernels of the other batch, 10-20 ms apiece)

    # ---- bitmap -> bins (index.py:438-465): what the viewer does with a queried bitmap ----
    @property
    def bitsum_index(self):
        return pd.RangeIndex(0, self.ngenomes + 1)

    @staticmethod
    def _bin_ids(bitmap: pd.DataFrame, binlen: int):
        bins = np.asarray(bitmap.index) // binlen
        ub, inv = np.unique(bins, return_inverse=True)
        return ub, inv

    def bitmap_to_bins(self, bitmap: pd.DataFrame, binlen: int):
        """(pancount_bins, paircount_bins) of a positions x genomes 0/1 bitmap: rows = occupancy 0..N
        and columns = bin number; rows = genomes and columns = bin start, every bin scaled by its
        largest genome count (index.py:438-449)."""
        ub, inv = self._bin_ids(bitmap, binlen)
        vals = bitmap.to_numpy()
        N = self.ngenomes
        flat = np.bincount(inv * (N + 1) + vals.sum(axis=1).astype(np.int64), minlength=len(ub) * (N + 1))
        pan = pd.DataFrame(flat.reshape(len(ub), N + 1).T, index=self.bitsum_index, columns=ub)
        return pan, self._paircount_bins(vals, ub, inv, binlen, bitmap.columns)

    @staticmethod
    def _paircount_bins(vals, ub, inv, binlen, columns):
        sums = np.zeros((len(ub), vals.shape[1]), np.int64)
        np.add.at(sums, inv, vals.astype(np.int64))
        pc = pd.DataFrame(sums.T, index=columns, columns=ub * binlen)
        return pc.div(pc.max(axis=0), axis=1)

    def bitmap_to_paircount_bins(self, bitmap: pd.DataFrame, binlen: int):
        ub, inv = self._bin_ids(bitmap, binlen)
        return self._paircount_bins(bitmap.to_numpy(), ub, inv, binlen, bitmap.columns)

    def bitmap_to_pancount(self, bitmap: pd.DataFrame) -> pd.Series:
        return pd.Series(bitmap.to_numpy().sum(axis=1), index=bitmap.index)

    def pancount_to_bins(self, pancnts: pd.Series, binlen: int) -> pd.DataFrame:
        bins = np.asarray(pancnts.index) // binlen
        ub, inv = np.unique(bins, return_inverse=True)
        N = self.ngenomes
        flat = np.bincount(inv * (N + 1) + pancnts.to_numpy().astype(np.int64), minlength=len(ub) * (N + 1))
        return pd.DataFrame(flat.reshape(len(ub), N + 1).T, index=self.bitsum_index, columns=ub)

    def query_genes(self, genome, chrom=None, start=None, end=None) -> pd.DataFrame:
        """the gene track's rows of ``genome`` overlapping the region (index.py:865-889): chr start end name, then the
        gene's positions held by 1 genome and by all N"""
        return self.genomes[genome].query_genes(chrom, start, end)

    def query_anno(self, genome, chrom, start, end) -> pd.DataFrame:
        """the annotation track's rows of ``genome`` overlapping the region (index.py:891-920), with ``type_id``"""
        return self.genomes[genome].query_anno(chrom, start, end)

    def query_bitmap(self, genome, chrom, start=None, end=None, step=1):
        return self.genomes[genome].query(chrom, start, end, step)

    def pair_counts(self, genome, chrom=None, start=None, end=None, step=1) -> pd.DataFrame:
        """N x N pair counts of the genomes over the rows ``query_bitmap(genome, chrom, start, end, step)`` returns"""
        return self.genomes[genome].pair_counts(chrom, start, end, step)

    def find_pattern(self, genome, have, lack=(), min_have=None, max_lack=0, chrom=None, start=None, end=None, step=1,
                     min_len=1, max_gap=0) -> pd.DataFrame:
        """the runs of rows of ``query_bitmap(genome, chrom, start, end, step)`` that at least ``min_have`` of the ``have``
        genomes hold and at most ``max_lack`` of the ``lack`` genomes do (``Genome.find_pattern``)"""
        return self.genomes[genome].find_pattern(have, lack, min_have, max_lack, chrom, start, end, step, min_len, max_gap)

    def pattern_density(self, genome, have, lack=(), min_have=None, max_lack=0, chroms=None, step=1,
                        bin_size=1_000_000) -> pd.DataFrame:
        """the matching rows of every bin of ``bin_size`` positions (``Genome.pattern_density``)"""
        return self.genomes[genome].pattern_density(have, lack, min_have, max_lack, chroms, step, bin_size)

    def pattern_counts(self, genome, genomes=None, chrom=None, start=None, end=None, step=1):
        """(keys, counts, selected names): the pattern spectrum of ``query_bitmap(genome, chrom, start, end, step)``'s rows over
        the ``genomes`` selected (``Genome.pattern_counts``)"""
        return self.genomes[genome].pattern_counts(genomes, chrom, start, end, step)

    def pattern_spectrum(self, genome, genomes=None, chrom=None, start=None, end=None, step=1, top=None, min_rows=1) -> pd.DataFrame:
        """the presence/absence patterns of the rows of ``query_bitmap(genome, chrom, start, end, step)`` and the rows each
        holds (``Genome.pattern_spectrum``)"""
        return self.genomes[genome].pattern_spectrum(genomes, chrom, start, end, step, top, min_rows)

    def absence_runs(self, genome, genomes=None, chrom=None, start=None, end=None, step=1, min_len=1, max_len=0) -> pd.DataFrame:
        """per genome of ``genomes``, the closed runs of rows of ``query_bitmap(genome, chrom, start, end, step)`` that lack its
        bit, with their candidate class at step 1 (``Genome.absence_runs``)"""
        return self.genomes[genome].absence_runs(genomes, chrom, start, end, step, min_len, max_len)

    def absence_spectrum(self, genome, genomes=None, chrom=None, start=None, end=None, step=1, maxlen=None) -> pd.DataFrame:
        """the closed absence runs of every length that each genome of ``genomes`` has in the rows of
        ``query_bitmap(genome, chrom, start, end, step)`` (``Genome.absence_spectrum``)"""
        return self.genomes[genome].absence_spectrum(genomes, chrom, start, end, step, maxlen)

    def search(self, queries, genomes=None, min_frac: float = 0.0, by: str = "kmers", batch_bases: Optional[int] = None):
        """(long, matrix, summary) — ``search.frames`` — of query sequences that are NOT in the index: which of the ``genomes``
        (names; None: all) carry each query, and how completely.  ``queries``: a FASTA path (plain or ``.gz``), FASTA bytes, or
        a list of (name, sequence).  Per query and genome: the query's k-mers the genome holds (``hits``, ``frac`` of the
        query's k-mers), the query's bases inside at least one held k-mer (``covered``, ``cov_frac`` of its length), the runs
        of held k-mers, the longest, the first held k-mer and one past the last.  ``min_frac`` drops lines of the long table
        below it; ``by="bases"`` makes ``cov_frac`` the value that ``min_frac``, the matrix and ``best`` go by.
        The query's k-mers are probed against the table of every sample's k-mers (built from the samples' sequence files
        on first use and cached), ``batch_bases`` bases at a time (``search.BATCH_BASES``; batches are cut between records, a
        longer record is a batch of its own), and their rows are reduced on the GPU (k_presence_profile).  A query shorter than
        k is reported with zeros.  A k-mer that holds a non-ACGT base is a row of zeros — held by no genome — as everywhere
        in the project: it counts in ``kmers`` and in ``none``, and cuts runs.  Queries stay in file order; duplicate names
        are kept.  KeyError: an unknown genome name."""
        from . import search as srch
        names = list(self.genome_names)
        cols = srch.pick_genomes(names, genomes)
        if by not in ("kmers", "bases"):
            raise ValueError(f"search: by must be 'kmers' or 'bases', got {by!r}")
        text, qnames, qlens, offs = srch.read_queries(queries)
        k, nq, N = int(self.k), len(qnames), len(names)
        profile, rows = np.zeros((nq, N, len(srch.FIELDS)), np.uint32), np.zeros((nq, 2), np.uint32)
        words = np.zeros((N + 31) // 32, np.uint32)
        for c in cols:
            words[c // 32] |= np.uint32(1 << (c % 32))
        todo = [(i, j) for i, j in srch.batches(qlens, srch.BATCH_BASES if batch_bases is None else batch_bases) if (qlens[i:j] >= k).any()]
        table = self._full_table() if todo and cols else None
        for i, j in todo if table is not None else []:
            at = i + np.flatnonzero(qlens[i:j] >= k)  # (a query shorter than k has no row: it stays on the host)
            whole = len(at) == j - i
            ss = engine.SeqSet.from_fasta(self.context, text[offs[i]:offs[j]] if whole else np.concatenate([text[offs[q]:offs[q + 1]] for q in at]))
            try:
                if list(ss.names) != [qnames[q] for q in at] or not np.array_equal(np.asarray(ss.lens, np.int64), qlens[at]):
                    raise RuntimeError(f"search: records {i} to {j} of the queries were read differently on the host and on the GPU")
                res = engine.AnchorResult(table, ss, colsums=False, rows_only=True)
                try:
                    res.run()
                    p, r = res.presence_profile(np.arange(len(at)), np.zeros(len(at), np.uint64), qlens[at] - k + 1, words)
                    profile[at], rows[at] = p, r
                finally:
                    res.close()
            finally:
                ss.close()
        return srch.frames(qnames, qlens, k, [names[c] for c in cols], profile[:, cols], rows, min_frac, by)

    def copies(self, targets, genomes=None, k=None, track: bool = False):
        """(long, matrix, summary) — ``copies.frames`` — of target sequences: how many copies of each target the assemblies of
        the ``genomes`` (names; None: all) hold.  ``targets``: a FASTA path (plain or ``.gz``), FASTA bytes, or a list of (name,
        sequence).  Per target and genome: the histogram of the depth — how often the genome holds the canonical k-mer — over
        the target's valid k-mer positions, reduced to ``present``, ``copies`` (its lower median), ``copies_nz``, ``mean`` and
        ``max_bin``.  ``track=True`` adds a fourth value, the depth of every position [genomes, the targets' k-mer positions back
        to back] (``copies.track_lines`` prints its runs).
        One count table is sized from the targets' k-mer positions (``engine.CopyTable``); the genomes are taken in batches of
        as many planes as the free memory holds, each streamed once through the table (k_copy_count) from its packed assembly
        (``seqset_for``; dropped again when this call loaded it), the batch's histograms taken in one pass over the targets
        (k_copy_profile).  A target shorter than k, or without a valid window, is reported with zeros.  Targets stay in order;
        duplicate names are kept.  KeyError: an unknown genome name; ValueError: a genome without an assembly FASTA (a FASTQ
        sample, or no sequence file), k outside 1..32."""
        from . import copies as cp, search as srch
        names = list(self.genome_names)
        cols = srch.pick_genomes(names, genomes)
        k = int(self.k) if k is None else int(k)
        if not 1 <= k <= 32:
            raise ValueError(f"copies: k={k} (1 to 32)")
        chosen = [names[c] for c in cols]
        for g in chosen:
            fa = self.genomes[g].fasta
            if fa is None or pd.isna(fa) or is_fastq(fa):
                raise ValueError(f"copies: genome {g!r} has no assembly FASTA to count k-mers in ({fa})")
        text, tnames, tlens, offs = srch.read_queries(targets)
        nt, ng = len(tnames), len(chosen)
        total = int(np.maximum(tlens - k + 1, 0).sum())
        hist, valid = np.zeros((nt, ng, cp.BINS), np.uint64), np.zeros(nt, np.uint64)
        depths = np.full((ng, total), cp.DEPTH_INVALID, np.uint16) if track else None
        if total and ng:
            at = np.flatnonzero(tlens >= k)  # (a target shorter than k has no position: it stays on the host)
            tss = engine.SeqSet.from_fasta(self.context, text if len(at) == nt else np.concatenate([text[offs[t]:offs[t + 1]] for t in at]))
            table = None
            try:
                if list(tss.names) != [tnames[t] for t in at] or not np.array_equal(np.asarray(tss.lens, np.int64), tlens[at]):
                    raise RuntimeError("copies: the targets were read differently on the host and on the GPU")
                per = cp.planes_for(self.context.mem_info()[0], cp.table_slots(total), ng, total if track else 0)
                table = engine.CopyTable(self.context, k, total, per)
                table.insert(tss)
                for g0 in range(0, ng, per):
                    batch = chosen[g0:g0 + per]
                    for plane, g in enumerate(batch):
                        if g0:
                            table.clear(plane)
                        mine = g not in self._seqsets
                        try:
                            table.count(plane, self.seqset_for(g))
                        finally:
                            if mine:
                                self.drop_seqset(g)
                    got = table.profile(tss, 0, len(batch), track)
                    hist[at, g0:g0 + len(batch)], valid[at] = got[0], got[1]
                    if track:
                        depths[g0:g0 + len(batch)] = got[2]
            finally:
                if table is not None:
                    table.close()
                tss.close()
        out = cp.frames(tnames, tlens, k, chosen, hist, valid)
        return (*out, depths) if track else out

    def place(self, anchor: str, reads, chroms=None, bin_size: int = 100000, min_count: int = 2, genomes=None,
              batch_bytes: Optional[int] = None):
        """(main, matrix, summary, stats) — ``place.frames`` — of an unassembled sample along the anchor genome ``anchor``: per bin
        of ``bin_size`` positions which of the indexed genomes the sample resembles.  ``reads``: FASTQ paths (plain or ``.gz``,
        four lines per record).  The comparison is about the index's k-mers: a k-mer of the anchor counts as held by the sample
        when the reads hold it at least ``min_count`` times (both strands; the only error filter), and per bin and genome the
        Jaccard index of the sample's column and the genome's is taken over the anchor's valid positions.  ``genomes`` (names;
        None: all): the genomes that take part — the anchor's own column included, a sample that is the anchor is called the
        anchor.  The GPU side is ``Genome.place_counts``: the read files are read again for every batch of the anchor's
        chromosomes.  KeyError: an unknown anchor, chromosome or genome; ValueError: a FASTQ anchor, an anchor without
        bitmap.1, a FASTA that disagrees with chrs.tsv, a missing read file, a torn last record."""
        from . import place as pl
        if anchor not in self.genomes:
            raise KeyError(f"place: unknown genome {anchor!r} (the index has {', '.join(self.genome_names)})")
        names = list(self.genome_names)
        pl.pick_columns(names, genomes)  # (refused before any work)
        bins, valid, held, col, both, stats = self[anchor].place_counts(reads, chroms, bin_size, min_count, batch_bytes)
        return (*pl.frames(bins, valid, held, col, both, names, genomes), stats)

    def screen(self, samples, min_count: Optional[int] = None, genomes=None, batch_bytes: Optional[int] = None):
        """(main, occupancy, stats) — ``screen.frames`` — of ONE sample from outside the index: which of the indexed genomes it
        holds, how much of each it recovers, whose private k-mers it carries, how deep it is sequenced and how much of it is in no
        indexed genome.  ``samples``: the sample's files, FASTQ (four lines per record) or FASTA, plain or ``.gz``, streamed one
        after the other; each is read ONCE.  The sample's k-mers are counted per k-mer of the table of every sample's k-mers
        (built from the samples' sequence files on first use and cached; ``engine.TableScreen``): FASTQ text ``batch_bytes`` at
        a time, joined on the GPU; a FASTA as one sequence set.  A k-mer is seen when the sample holds it at least ``min_count``
        times (1 to 255; None: 2 when any file is FASTQ, else 1).  ``genomes`` (names; None: all) selects the lines of the main
        table only: ranks are among all genomes.  ``stats["novel_frac"]`` counts window instances, sequencing errors among them.
        KeyError: an unknown genome name; ValueError: a missing file, a torn last record, a ``min_count`` outside 1..255;
        RuntimeError: the cached table holds some anchors' k-mers only."""
        from . import place as pl, screen as scr
        names = list(self.genome_names)
        scr.pick_genomes(names, genomes)  # (refused before any work)
        samples = [samples] if isinstance(samples, (str, os.PathLike)) else list(samples)
        paths = [os.fspath(p) for p in samples]
        for p in paths:
            if not os.path.isfile(p):
                raise ValueError(f"screen: no sample file {p!r}")
        min_count = scr.check_min_count(scr.default_min_count(any(is_fastq(p) for p in paths)) if min_count is None else min_count)
        batch_bytes = pl.DEFAULT_BATCH_BYTES if batch_bytes is None else int(batch_bytes)
        if batch_bytes < 1:
            raise ValueError(f"screen: batch_bytes must be positive, got {batch_bytes}")
        ctx = self.context
        sc = engine.TableScreen(self._full_table())
        tot = {"windows": 0, "hits": 0, "reads": 0, "read_bases": 0}

        def add(ss, reads, bases):
            w, h = sc.add(ss)
            for f, v in (("windows", w), ("hits", h), ("reads", reads), ("read_bases", bases)):
                tot[f] += int(v)
        try:
            for p in paths:
                if is_fastq(p):
                    fb = pl.FastqBatches(p, batch_bytes)
                    for buf in fb:
                        rs, n, used = engine.SeqSet.from_fastq(ctx, buf)
                        try:
                            add(rs, n, int(rs.lens[0]) - max(n - 1, 0))
                        finally:
                            rs.close()
                        fb.advance(used)
                else:
                    ss = engine.SeqSet.from_fasta(ctx, p)
                    try:
                        add(ss, len(ss.lens), int(np.asarray(ss.lens, np.uint64).sum()))
                    finally:
                        ss.close()
            counts = sc.result(min_count)
        finally:
            sc.close()
        return scr.frames(counts, names, int(self.k), min_count, tot["windows"], tot["hits"], tot["reads"], tot["read_bases"], genomes)

    def novel(self, samples, min_count: Optional[int] = None, batch_bytes: Optional[int] = None, kmers: bool = False,
              regions: bool = False, min_bases: int = 0, unitigs: bool = False, min_unitig_bases: int = 0, clean: Optional[dict] = None):
        """(stats, spectrum, kmers, regions) — ``novel.stats``, ``novel.spectrum_frame``, ``novel.kmers_frame`` (None unless
        ``kmers``), ``novel.regions_frame`` filtered by ``min_bases`` (None unless ``regions``) — of ONE sample from outside the
        index: the distinct k-mers it holds that NO indexed genome does, their depth spectrum, and for an assembly where they
        lie.  ``samples``, ``batch_bytes`` and the default of ``min_count`` as ``screen`` takes them; the sample is streamed once
        through the table of every sample's k-mers and its missing windows are counted in a table of their own that grows on the
        GPU (``engine.NovelTable``).  A k-mer is solid when the sample holds it at least ``min_count`` times — the only error
        filter.  With ``unitigs`` a fifth value follows: ``novel.unitigs_frame`` — the solid k-mers compacted on the GPU into the
        non-branching paths of their de Bruijn graph (``engine.NovelTable.unitigs``: an insertion is one unitig, a plasmid a
        circular one), those of at least ``min_unitig_bases`` bases — from the same novel table, the sample still streamed once.
        ``clean`` (needs ``unitigs``; a dict of ``tip_kmers``, ``bubble_kmers``, ``ratio``, ``rounds``, each optional): error tips
        are clipped and bubbles popped on the GPU before the compaction (``engine.NovelTable.clean``), and a sixth value follows:
        its statistics, ``novel.CLEAN_STAT_NAMES``.
        ValueError: a missing file, a torn last record, ``min_count`` outside 1..2^32 - 1, a negative ``min_bases`` or
        ``min_unitig_bases``, ``regions`` with a FASTQ file (regions need an assembly); RuntimeError: the cached table holds some
        anchors' k-mers only."""
        from . import novel as nov, place as pl
        samples = [samples] if isinstance(samples, (str, os.PathLike)) else list(samples)
        paths = [os.fspath(p) for p in samples]
        for p in paths:
            if not os.path.isfile(p):
                raise ValueError(f"novel: no sample file {p!r}")
        if regions and any(is_fastq(p) for p in paths):
            raise ValueError("novel: regions need an assembly: " + ", ".join(repr(p) for p in paths if is_fastq(p)) + " is FASTQ")
        if int(min_bases) < 0:
            raise ValueError(f"novel: min_bases={min_bases} must not be negative")
        if int(min_unitig_bases) < 0:
            raise ValueError(f"novel: min_unitig_bases={min_unitig_bases} must not be negative")
        if clean is not None:
            if not unitigs:
                raise ValueError("novel: clean needs unitigs")
            try:
                clean = nov.clean_options(int(self.k), **clean)
            except (TypeError, ValueError) as e:
                raise ValueError(f"novel: clean: {e}") from None
        min_count = nov.check_min_count(nov.default_min_count(any(is_fastq(p) for p in paths)) if min_count is None else min_count)
        batch_bytes = pl.DEFAULT_BATCH_BYTES if batch_bytes is None else int(batch_bytes)
        if batch_bytes < 1:
            raise ValueError(f"novel: batch_bytes must be positive, got {batch_bytes}")
        ctx, k = self.context, int(self.k)
        table = self._full_table()
        nt = engine.NovelTable(table)
        tot = {"windows": 0, "hits": 0, "reads": 0, "read_bases": 0}
        found = []

        def add(ss, reads, bases):
            w, h, _ = nt.add(ss)
            for f, v in (("windows", w), ("hits", h), ("reads", reads), ("read_bases", bases)):
                tot[f] += int(v)
        try:
            for p in paths:
                if is_fastq(p):
                    fb = pl.FastqBatches(p, batch_bytes)
                    for buf in fb:
                        rs, n, used = engine.SeqSet.from_fastq(ctx, buf)
                        try:
                            add(rs, n, int(rs.lens[0]) - max(n - 1, 0))
                        finally:
                            rs.close()
                        fb.advance(used)
                else:
                    ss = engine.SeqSet.from_fasta(ctx, p)
                    try:
                        add(ss, len(ss.lens), int(np.asarray(ss.lens, np.uint64).sum()))
                        if regions:
                            found.append(nov.regions_frame(p, ss.names, *engine.novel_runs(table, ss)[:5], k))
                    finally:
                        ss.close()
            counts = nt.result(min_count)
            kmers_df = nov.kmers_frame(*nt.keys(min_count), k) if kmers else None
            if unitigs:
                if clean is not None:
                    clean_stats = nt.clean(min_count, **clean)
                u = nt.unitigs(min_count)
                unitigs_df = nov.unitigs_frame(u["offsets"], u["kmers"], u["depth_sum"], u["circular"], u["bases"], k, min_unitig_bases)
        finally:
            nt.close()
        regions_df = nov.filter_regions(pd.concat(found, ignore_index=True) if found else nov.no_regions(), min_bases) if regions else None
        st = nov.stats(counts, min_count, tot["windows"], tot["hits"], tot["reads"], tot["read_bases"], regions_df)
        if unitigs and clean is not None:
            return st, nov.spectrum_frame(counts["depth_hist"]), kmers_df, regions_df, unitigs_df, clean_stats
        if unitigs:
            return st, nov.spectrum_frame(counts["depth_hist"]), kmers_df, regions_df, unitigs_df
        return st, nov.spectrum_frame(counts["depth_hist"]), kmers_df, regions_df

    def locate(self, queries, genomes=None, k=None, min_run: int = 1, max_gap: int = 1000, max_shift: int = 100, min_kmers: int = 1,
               min_frac: float = 0.0):
        """(loci, matrix, summary) — ``locate.frames`` — of query sequences: WHERE each lies in the assemblies of the ``genomes``
        (names; None: all) — chromosome, start, end, strand, every copy.  ``queries``: a FASTA path (plain or ``.gz``), FASTA
        bytes, or a list of (name, sequence).  A locus is a block of collinear hits (``synteny --blocks``' chaining with
        ``min_run``, ``max_gap``, ``max_shift``; the genome is A, the queries are B) of k-mers that occur exactly once among the
        queries, however often the genome holds them; ``frac`` = its k-mers / the query's unique k-mers; ``min_kmers`` and
        ``min_frac`` drop loci below them.
        One position table is sized from the queries' k-mer positions and the queries are inserted once (``engine.PosTable``,
        side 1); the queries streamed through it give ``unique``; then every genome is streamed once from its packed assembly
        (``seqset_for``; dropped again when this call loaded it) and only its blocks leave the GPU (k_hit_runs, k_run_blocks).
        A query shorter than k stays in matrix and summary with zeros.  Queries stay in order; duplicate names are kept.  The
        chromosomes' lengths ride in ``loci.attrs["chrom_lens"]`` (genome -> chromosome -> bases) for ``locate.paf_lines``.
        KeyError: an unknown genome name; ValueError: a genome without an assembly FASTA (a FASTQ sample, or no sequence file),
        k outside 1..32, a parameter outside its range."""
        from . import locate as loc, search as srch
        names = list(self.genome_names)
        cols = srch.pick_genomes(names, genomes)
        k = int(self.k) if k is None else int(k)
        if not 1 <= k <= 32:
            raise ValueError(f"locate: k={k} (1 to 32)")
        for name, v, lo in (("min_run", min_run, 1), ("max_gap", max_gap, 1), ("max_shift", max_shift, 0)):
            if not lo <= int(v) <= 0x7FFFFFFF:
                raise ValueError(f"locate: {name}={v} ({lo} to 2^31 - 1)")
        if int(min_kmers) < 1 or not 0.0 <= float(min_frac) <= 1.0:
            raise ValueError(f"locate: min_kmers={min_kmers} (at least 1), min_frac={min_frac} (0 to 1)")
        chosen = [names[c] for c in cols]
        for g in chosen:
            fa = self.genomes[g].fasta
            if fa is None or pd.isna(fa) or is_fastq(fa):
                raise ValueError(f"locate: genome {g!r} has no assembly FASTA to look in ({fa})")
        text, qnames, qlens, offs = srch.read_queries(queries)
        nq = len(qnames)
        total = int(np.maximum(qlens - k + 1, 0).sum())
        unique = np.zeros(nq, np.int64)
        per_genome, chrom_lens = [], {}
        at = np.flatnonzero(qlens >= k)  # (a query shorter than k has no position: it stays on the host)
        if total and chosen:
            qss = engine.SeqSet.from_fasta(self.context, text if len(at) == nq else np.concatenate([text[offs[q]:offs[q + 1]] for q in at]))
            table = None
            try:
                if list(qss.names) != [qnames[q] for q in at] or not np.array_equal(np.asarray(qss.lens, np.int64), qlens[at]):
                    raise RuntimeError("locate: the queries were read differently on the host and on the GPU")
                table = engine.PosTable(self.context, k, total)
                table.insert(1, qss)
                unique[at] = table.hit_runs(qss)[5]
                for g in chosen:
                    mine = g not in self._seqsets
                    try:
                        ss = self.seqset_for(g)
                        got = table.locate(ss, qss, min_run, max_gap, max_shift)
                        blk = loc.genome_loci(got[:8], k, len(ss.lens), qlens[at])
                        blk["chrB"] = at[blk["chrB"].to_numpy(np.int64)]  # (the query's number among all of them)
                        per_genome.append((list(ss.names), blk))
                        chrom_lens[g] = dict(zip(ss.names, (int(n) for n in ss.lens)))
                    finally:
                        if mine:
                            self.drop_seqset(g)
            finally:
                if table is not None:
                    table.close()
                qss.close()
        else:
            per_genome = [([], loc.genome_loci([np.zeros(0, np.uint32)] * 8, k, 0, [])) for _ in chosen]
        loci, matrix, summary = loc.frames(qnames, qlens, k, unique, chosen, per_genome, min_kmers, min_frac)
        loci.attrs["chrom_lens"] = chrom_lens
        return loci, matrix, summary

    def _synteny_sides(self, a, b, chroms_a, chroms_b, k, run):
        """``run(k, seqs_a, seqs_b)`` on the two genomes' sequence sets, narrowed to the chosen chromosomes: (its result, k, per
        side (names, lengths) of the chromosomes taken)"""
        from . import synteny
        k = int(self.k) if k is None else int(k)
        if not 1 <= k <= 32:
            raise ValueError(f"synteny: k={k} (1 to 32)")
        for g in (a, b):
            if g not in self.genomes:
                raise KeyError(f"synteny: unknown genome {g!r} (the index has {', '.join(self.genome_names)})")
        sides, made = [], []
        try:
            for g, chosen in ((a, chroms_a), (b, chroms_b)):
                ss = self.seqset_for(g)
                names = list(ss.names)
                pick = synteny.pick_contigs(names, chosen)
                if chosen is not None:  # (whole contigs: a piece of its contig's full length from base 0)
                    ss = ss.slice([(c, 0, int(ss.lens[c])) for c in pick])
                    made.append(ss)
                sides.append((ss, [names[c] for c in pick], [int(self.seqset_for(g).lens[c]) for c in pick]))
            (ss_a, names_a, lens_a), (ss_b, names_b, lens_b) = sides
            got = run(k, ss_a, ss_b)
        finally:
            for ss in made:
                ss.close()
        return got, k, (names_a, lens_a), (names_b, lens_b)

    def synteny_tables(self, a, b, chroms_a=None, chroms_b=None, k=None, min_len=1):
        """(segments, summary, totals) of ``synteny``: the summary is ``synteny.summary_frame`` of the segments; the totals
        (``synteny.totals_frame``) give per side the positions whose k-mer is unique in that genome — each side against itself,
        two more passes that emit nothing — and those with a mate in the other"""
        from . import synteny

        def run(k, ss_a, ss_b):
            rc, rs, re_, rm, _, nmated = engine.synteny_segments(self.context, k, ss_a, ss_b)
            return rc, rs, re_, rm, nmated, [engine.synteny_counts(self.context, k, ss, ss)[1] for ss in (ss_a, ss_b)]
        (rc, rs, re_, rm, nmated, unique), k, (names_a, _), (names_b, lens_b) = self._synteny_sides(a, b, chroms_a, chroms_b, k, run)
        seg = synteny.segment_frame(rc, rs, re_, rm, k, names_a, lens_b, names_b, min_len)
        return seg, synteny.summary_frame(seg), synteny.totals_frame(a, b, unique[0], unique[1], nmated)

    def synteny_blocks_tables(self, a, b, chroms_a=None, chroms_b=None, k=None, min_run=1, max_gap=1000, max_shift=100, min_len=1):
        """(blocks, summary, totals, lengths) of ``synteny --blocks``: the runs of ``synteny_tables`` chained on the GPU into
        blocks that bridge substitutions and small insertions and deletions (``engine.synteny_blocks``; the runs never leave
        HBM) as ``synteny.block_frame`` lays them out — ``min_len`` drops blocks of fewer k-mers; summary and totals as
        ``synteny_tables``; lengths = per side a dict chromosome -> bases, what ``synteny.paf_lines`` takes"""
        from . import synteny
        for name, v, lo in (("min_run", min_run, 1), ("max_gap", max_gap, 1), ("max_shift", max_shift, 0)):
            if not lo <= int(v) <= 0x7FFFFFFF:
                raise ValueError(f"synteny: {name}={v} ({lo} to 2^31 - 1)")

        def run(k, ss_a, ss_b):
            got = engine.synteny_blocks(self.context, k, ss_a, ss_b, min_run, max_gap, max_shift)
            return got, [engine.synteny_counts(self.context, k, ss, ss)[1] for ss in (ss_a, ss_b)]
        (got, unique), k, (names_a, lens_a), (names_b, lens_b) = self._synteny_sides(a, b, chroms_a, chroms_b, k, run)
        blk = synteny.block_frame(*got[:8], k, names_a, lens_b, names_b, min_len)
        return (blk, synteny.summary_frame(blk), synteny.totals_frame(a, b, unique[0], unique[1], got[9]),
                (dict(zip(names_a, lens_a)), dict(zip(names_b, lens_b))))

    def synteny_variants_tables(self, a, b, chroms_a=None, chroms_b=None, k=None, min_run=1, max_gap=1000, max_shift=100):
        """(variants, class summary, totals, lengths) of ``synteny --variants``: every link of the blocks of
        ``synteny_blocks_tables`` classified and compared base by base on the GPU (``engine.synteny_variants``; runs and blocks
        never leave HBM) as ``synteny.variant_frame`` lays them out — the SNPs, insertions and deletions of ``b`` against ``a``
        with both alleles; the class summary is ``synteny.variant_summary_frame``; totals and lengths as
        ``synteny_blocks_tables``"""
        from . import synteny
        for name, v, lo, hi in (("min_run", min_run, 1, 0x7FFFFFFF), ("max_gap", max_gap, 1, 65536), ("max_shift", max_shift, 0, 0x7FFFFFFF)):
            if not lo <= int(v) <= hi:
                raise ValueError(f"synteny: {name}={v} ({lo} to {hi})")

        def run(k, ss_a, ss_b):
            got = engine.synteny_variants(self.context, k, ss_a, ss_b, min_run, max_gap, max_shift)
            # (long and N-flagged alleles are cut from the sets while they live; the chromosomes are numbered here and named below:
            # a narrowed side's set names its pieces, not its chromosomes)
            frame = synteny.variant_frame(*got[:9], range(len(ss_a.lens)), [int(n) for n in ss_b.lens], range(len(ss_b.lens)), ss_a, ss_b)
            return got, frame, [engine.synteny_counts(self.context, k, ss, ss)[1] for ss in (ss_a, ss_b)]
        (got, frame, unique), k, (names_a, lens_a), (names_b, lens_b) = self._synteny_sides(a, b, chroms_a, chroms_b, k, run)
        for col, names in (("chrA", names_a), ("chrB", names_b)):
            frame[col] = np.asarray(list(names), object)[frame[col].to_numpy(np.int64)] if len(frame) else np.zeros(0, object)
        return (frame, synteny.variant_summary_frame(frame, got[9], got[10]), synteny.totals_frame(a, b, unique[0], unique[1], got[11]),
                (dict(zip(names_a, lens_a)), dict(zip(names_b, lens_b))))

    def synteny(self, a, b, chroms_a=None, chroms_b=None, k=None, min_len=1) -> pd.DataFrame:
        """The maximal collinear runs of k-mers that occur exactly once in genome ``a`` and exactly once in genome ``b`` — the
        unique-match segments of a dot plot — found on the GPU from the two genomes' packed sequences: columns ``chrA startA
        endA chrB startB endB strand kmers``, half-open base ranges, sorted by (chromosome of ``a`` in file order, startA).
        ``chroms_a`` / ``chroms_b`` narrow a side to some chromosomes (uniqueness is then judged among those); ``k`` defaults to
        the index's (any 1..32: the table of all samples' k-mers is not read); ``min_len`` drops runs of fewer k-mers.  Not an
        alignment: a single mismatch ends a segment; ``synteny_blocks_tables`` chains the segments into blocks."""
        return self.synteny_tables(a, b, chroms_a, chroms_b, k, min_len)[0]

    def genotype(self, a, b, samples, chroms_a=None, chroms_b=None, k=None, min_run=1, max_gap=1000, max_shift=100, min_count=None,
                 min_frac=0.5, batch_bytes: Optional[int] = None):
        """(table, summary, stats) — ``genotype.frames`` and ``genotype.stats`` — of ONE sample from outside the index at every
        variant of genome ``b`` against genome ``a``: which allele it carries.  The variants are those of
        ``synteny_variants_tables`` with the same arguments.  The k-mers that span either allele of every variant go into a count
        table of three planes (``engine.CopyTable.insert_ranges``: no contig is cut per variant); plane 0 is counted from the
        WHOLE assembly of ``a`` and plane 1 from the whole assembly of ``b``, also when ``chroms_a`` / ``chroms_b`` narrowed the
        variant calling — the sample's reads come from the whole genome, so uniqueness is judged against all of it; the sample
        is streamed into plane 2 as ``screen`` streams it (``samples``, ``batch_bytes`` and the default of ``min_count`` as
        there); and ``engine.CopyTable.allele_support`` reduces the planes along A's alleles and along B's to four integers per
        variant and side.  The call rule with ``min_frac`` is ``genotype.call``'s.  ValueError: ``a == b``, a genome without an
        assembly FASTA, a missing sample file, ``min_frac`` outside (0, 1], ``min_count`` below 1, what ``synteny_variants_tables``
        refuses; KeyError: an unknown genome."""
        from . import genotype as gt, place as pl, screen as scr
        for g in (a, b):
            if g not in self.genomes:
                raise KeyError(f"genotype: unknown genome {g!r} (the index has {', '.join(self.genome_names)})")
        if a == b:
            raise ValueError(f"genotype: {a!r} against itself has no variants")
        for g in (a, b):
            fa = self.genomes[g].fasta
            if pd.isna(fa) or is_fastq(str(fa)) or not os.path.isfile(str(fa)):
                raise ValueError(f"genotype: genome {g!r} has no assembly FASTA ({fa})")
        samples = [samples] if isinstance(samples, (str, os.PathLike)) else list(samples)
        paths = [os.fspath(p) for p in samples]
        for p in paths:
            if not os.path.isfile(p):
                raise ValueError(f"genotype: no sample file {p!r}")
        min_frac = gt.check_min_frac(min_frac)
        min_count = gt.check_min_count(scr.default_min_count(any(is_fastq(p) for p in paths)) if min_count is None else min_count)
        batch_bytes = pl.DEFAULT_BATCH_BYTES if batch_bytes is None else int(batch_bytes)
        if batch_bytes < 1:
            raise ValueError(f"genotype: batch_bytes must be positive, got {batch_bytes}")
        variants = self.synteny_variants_tables(a, b, chroms_a, chroms_b, k, min_run, max_gap, max_shift)[0]
        k = int(self.k) if k is None else int(k)
        ctx = self.context
        ss_a, ss_b = self.seqset_for(a), self.seqset_for(b)
        ranges_a, ranges_b = gt.allele_ranges(variants, list(ss_a.names), list(ss_b.names))
        zero = tuple(np.zeros(0, np.uint64) for _ in range(4))
        reads = hits = 0
        if len(variants):
            # a range of l bases has at most l + k - 1 windows: enough for the distinct keys of both sides
            capacity = sum(int(r[2].sum()) + (k - 1) * len(variants) for r in (ranges_a, ranges_b))
            table = engine.CopyTable(ctx, k, max(capacity, 1), 3)
            try:
                table.insert_ranges(ss_a, *ranges_a)
                table.insert_ranges(ss_b, *ranges_b)
                table.count(0, ss_a)
                table.count(1, ss_b)
                for p in paths:
                    if is_fastq(p):
                        fb = pl.FastqBatches(p, batch_bytes)
                        for buf in fb:
                            rs, n, used = engine.SeqSet.from_fastq(ctx, buf)
                            try:
                                hits += table.count(2, rs)
                                reads += int(n)
                            finally:
                                rs.close()
                            fb.advance(used)
                    else:
                        ss = engine.SeqSet.from_fasta(ctx, p)
                        try:
                            hits += table.count(2, ss)
                            reads += len(ss.lens)
                        finally:
                            ss.close()
                sup_a = table.allele_support(ss_a, *ranges_a, 0, 1, 2, min_count)
                sup_b = table.allele_support(ss_b, *ranges_b, 1, 0, 2, min_count)
            finally:
                table.close()
        else:
            sup_a = sup_b = zero
        out, summary = gt.frames(variants, sup_a, sup_b, min_frac)
        return out, summary, gt.stats(out, sup_a, sup_b, reads, hits, min_count, min_frac)

    def region_tree(self, genome, chrom, start=None, end=None, step=None) -> "RegionTree":
        """The tree of the genomes over a region, as the viewer draws it (view.py:751-764: create_tree) — but from the pair
        counts of EVERY row of the region at ``step`` (default: the low-resolution step), not from a random sample of
        50 000 rows, so the same region gives the same tree.  ``chrom=None``: the whole genome."""
        step = int(self.lowres_step) if step is None else int(step)
        counts, nrows = self.genomes[genome]._pair_counts(chrom, start, end, step)
        if nrows == 0:
            where = "the whole genome" if chrom is None else f"{chrom}:{0 if start is None else start}-{'' if end is None else end}"
            raise ValueError(f"{genome}: no rows in {where} at step {step}")
        return RegionTree.from_counts(counts, list(self.genome_names))

    def close(self):
        for nm in list(self._seqsets):
            self.drop_seqset(nm)
        if self._table is not None:
            self._table.close()
            self._table = None
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None


class Genome:
    """One sample (index.py:468-1189), write side = ``run_anchor``, read side = ``query``."""

    def __init__(self, idx: Index, id: int, name: str, fasta=None, gff=None, anchor=None, write=False):
        self.index = idx
        self.id = id
        self.name = name
        self.fasta = fasta
        self.gff = gff
        self.write_mode = write
        self.prefix = os.path.join(idx.prefix, ANCHOR_DIR, name)
        self.anchored = bool(anchor) if anchor is not None else (fasta is not None and not pd.isna(fasta))
        self.ngenomes = idx.ngenomes
        self.nbytes = int(np.ceil(self.ngenomes / 8))
        self.steps = list(idx.steps)
        self.chrs = None
        self.blocks = None
        # this genome's own log (logs/anchor.<name>.log.txt when set up): the reference ran one process — and so
        # one basicConfig — per genome; here many genomes share a process, each with a handler of its own
        self.log = logging.getLogger(f"{__name__}.genome.{name}")
        self._log_handler = None
        self._bench_t0 = None  # when this genome's anchoring began (write_benchmark)
        if self.anchored and os.path.exists(self.chrs_fname):
            self.load_chrs()

    @property
    def chrs_fname(self):
        return os.path.join(self.prefix, "chrs.tsv")

    @property
    def chr_genes_fname(self):
        return os.path.join(self.prefix, "bitsum.genes.tsv")

    @property
    def annotated(self) -> bool:
        return self.gff is not None and not pd.isna(self.gff)

    def load_genes(self) -> pd.DataFrame:
        """The GFF records whose type is a gene type (index.py:669-691,731-736), sorted by (chr,
        start); ``start`` / ``end`` are used as they stand in the file, like the reference does
        when it slices ``bitsum[start:end]`` (index.py:1056-1063)."""
        df = pd.read_csv(self.gff, sep="\t", comment="#", header=None,
                         names=["chr", "source", "type", "start", "end", "score", "strand", "phase", "attr"],
                         usecols=["chr", "type", "start", "end"], dtype={"chr": str})
        df = df[df["type"].isin(self.index.gff_gene_types)]
        return df.sort_values(["chr", "start"], kind="stable").reset_index(drop=True)

    def gene_copies(self, genomes=None, k=None, track: bool = False):
        """``Index.copies`` with this annotated anchor's genes as the targets: ``load_genes`` gives chromosome, start and end —
        bases [start, end) as they stand in the GFF, cut at the chromosome's end — and a gene is named ``chr:start-end``.  The
        genes are cut from the anchor's packed sequence set on the GPU (``SeqSet.slice``, whose pieces start at multiples of 32:
        the up to 31 bases in front are trimmed on the host).  A gene on a chromosome the FASTA lacks, or with end <= start, is an
        empty target: it stays in the tables with zeros.  ValueError: no GFF."""
        return self.index.copies(self._gene_targets("copies"), genomes, k, track)

    def gene_loci(self, genomes=None, k=None, min_run: int = 1, max_gap: int = 1000, max_shift: int = 100, min_kmers: int = 1,
                  min_frac: float = 0.0):
        """``Index.locate`` with this annotated anchor's genes as the queries, cut and named as ``gene_copies`` does: where every
        gene lies in the ``genomes``' assemblies.  ValueError: no GFF."""
        return self.index.locate(self._gene_targets("locate"), genomes, k, min_run, max_gap, max_shift, min_kmers, min_frac)

    def _gene_targets(self, what: str) -> list:
        """(name, sequence) of every gene of ``load_genes``, for ``gene_copies`` and ``gene_loci`` (``what``: the caller, for the
        error's text)"""
        from . import copies as cp
        if not self.annotated:
            raise ValueError(f"{what}: genome {self.name!r} has no GFF to take genes from")
        genes = self.load_genes()
        idx = self.index
        mine = self.name not in idx._seqsets
        ss = idx.seqset_for(self.name)
        try:
            contig = {n: i for i, n in reversed(list(enumerate(ss.names)))}
            spans = [(contig[c], max(0, int(s)), min(int(e), int(ss.lens[contig[c]]))) if c in contig else (0, 0, 0)
                     for c, s, e in zip(genes["chr"], genes["start"], genes["end"])]  # (a chromosome the FASTA lacks: an empty target)
            seqs = [b""] * len(spans)
            cut = [i for i, (_, s, e) in enumerate(spans) if e > s]
            if cut:
                pieces = ss.slice([(spans[i][0], spans[i][1] & ~31, spans[i][2] - (spans[i][1] & ~31)) for i in cut])
                try:
                    for j, i in enumerate(cut):
                        seqs[i] = pieces.unpack(j)[spans[i][1] & 31:]
                finally:
                    pieces.close()
        finally:
            if mine:
                idx.drop_seqset(self.name)
        return list(zip(cp.gene_names(genes), seqs))

    @property
    def bins_fname(self):
        return os.path.join(self.prefix, "bitsum.bins.tsv")

    def bitmap_gz_fname(self, step):
        return os.path.join(self.prefix, f"bitmap.{step}.{BGZ_SUFFIX}")

    def bitmap_gzi_fname(self, step):
        return os.path.join(self.prefix, f"bitmap.{step}.{IDX_SUFFIX}")

    @property
    def anchor_filenames(self):
        if not self.anchored:
            return []
        ret = [self.chrs_fname, self.bins_fname]
        for s in self.steps:
            ret += [self.bitmap_gz_fname(s), self.bitmap_gzi_fname(s)]
        return ret

    def iter_fasta(self):
        return read_fasta(self.fasta)

    # ---- chrs / offsets (index.py:576-604) ----
    def set_chrs(self, chrs: pd.DataFrame):
        self.chrs = chrs
        if "gene_count" not in self.chrs.columns:
            self.chrs["gene_count"] = 0
        self.sizes = chrs["size"]
        step_sizes = pd.DataFrame({step: np.ceil(self.sizes / step) for step in self.steps}, dtype=int)
        self.offsets = step_sizes.cumsum().shift(fill_value=0)

    def load_chrs(self):
        self.set_chrs(pd.read_table(self.chrs_fname, index_col="name"))

    # ---- WRITE: the hot path ----
    def setup_log(self, logfile: Optional[str]):
        """route this genome's messages to ``logfile`` (same line format as the reference's anchor logs)"""
        self.close_log()
        if logfile:
            h = logging.FileHandler(logfile)
            h.setFormatter(logging.Formatter("[ %(asctime)s %(levelname)7s ] %(message)s", datefmt="%Y-%m-%d %H:%M:%S"))
            self.log.addHandler(h)
            self.log.setLevel(logging.INFO)
            self._log_handler = h

    def write_benchmark(self) -> None:
        """logs/anchor.<name>.benchmark.txt in the format of Snakemake's ``benchmark:`` directive — the reference's own timing
        artefact for this step (panagram/workflow/Snakefile:43-44; cpp/Snakefile:43-44): one header line, one row, tab-separated
        ``s  h:m:s  max_rss  max_vms  max_uss  max_pss  io_in  io_out  mean_load  cpu_time`` (seconds; MB; percent).  The
        reference runs one process per anchor; here every anchor of a run shares one process per GPU, so ``s`` is the wall
        time from the moment this genome's anchoring began (its log's "Anchoring Started": the launch it shares with the
        other anchors of its batch) until its files were complete, and the memory / IO / CPU columns are the process's."""
        import resource
        import time
        if not self.index.write_mode:
            return
        t0 = self._bench_t0 if self._bench_t0 is not None else getattr(self.index, "_run_t0", None)
        if t0 is None:
            return
        secs = max(0.0, time.perf_counter() - t0)
        cpu = max(0.0, time.process_time() - getattr(self.index, "_cpu_t0", 0.0))
        rss = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0
        vms = uss = pss = io_in = io_out = float("nan")
        try:
            import psutil
            pr = psutil.Process()
            mi = pr.memory_full_info()
            vms, uss, pss = mi.vms / 2 ** 20, mi.uss / 2 ** 20, getattr(mi, "pss", float("nan")) / 2 ** 20
            io = pr.io_counters()
            io_in, io_out = io.read_chars / 2 ** 20, io.write_chars / 2 ** 20
        except Exception:  # noqa: BLE001 — psutil missing or /proc restricted: the columns stay NaN, as Snakemake writes them then
            pass
        hms = f"{int(secs // 3600)}:{int(secs % 3600 // 60):02d}:{int(secs % 60):02d}"
        os.makedirs(self.index.get_subdir("logs"), exist_ok=True)
        path = os.path.join(self.index.get_subdir("logs"), f"anchor.{self.name}.benchmark.txt")
        fields = [f"{secs:.4f}", hms] + [f"{x:.2f}" for x in (rss, vms, uss, pss, io_in, io_out, 100.0 * cpu / secs if secs > 0 else 0.0, cpu)]
        with open(path + ".tmp", "w") as f:
            f.write("s\th:m:s\tmax_rss\tmax_vms\tmax_uss\tmax_pss\tio_in\tio_out\tmean_load\tcpu_time\n" + "\t".join(fields) + "\n")
        os.replace(path + ".tmp", path)
        self._bench_t0 = None  # a second run of the same object counts from its own start

    def ensure_log(self, started: Optional[float] = None):
        """logs/anchor.<name>.log.txt, unless a log has been set up already.  ``started``: when this genome's anchoring
        began, if that was before this call (a genome assembled from pieces: its launches ran long before its log opens)"""
        if self._bench_t0 is None:
            import time
            self._bench_t0 = time.perf_counter() if started is None else started
        if self._log_handler is None and self.index.write_mode:
            os.makedirs(self.index.get_subdir("logs"), exist_ok=True)
            self.setup_log(os.path.join(self.index.get_subdir("logs"), f"anchor.{self.name}.log.txt"))

    def close_log(self):
        if self._log_handler is not None:
            self.log.removeHandler(self._log_handler)
            self._log_handler.close()
            self._log_handler = None

    def anchor_on_gpu(self, table: engine.PanTable, ss: engine.SeqSet):
        """Enqueue the anchor kernels for a packed FASTA and fetch the small outputs (bins, column
        sums); the bitmap rows stay in HBM for ``write_from_result``."""
        self.ensure_log()
        for nm, ln in zip(ss.names, ss.lens):
            if int(ln) < table.k:
                self.log.warning(f"Contig {nm} is shorter than k={table.k}: 0 k-mers (the reference underflows here)")
        self.log.info("Anchoring Started")
        res = engine.AnchorResult(table, ss, colsums=True, **self.index.result_geometry)
        res.run()
        return dict(res=res, merged=None, genomes=[self.tabulate(res, 0, len(ss.names), list(ss.names))])

    def tabulate(self, res, lo: int, hi: int, names: List[str]):
        """The small outputs of this genome's contigs ``lo..hi-1`` of a finished result — per-contig bins and
        geometry, column sums, per-gene occupancy — as the tuple ``write_from_result`` takes; the bitmap rows
        stay in HBM."""
        self.ensure_log()
        small = res.contigs_small(lo, hi - lo)  # (one call for all contigs; small[i] = what res.download(lo + i, False, False) gives)
        cs = res.contig_colsums(lo, hi - lo).astype(np.int64).sum(axis=0)
        gene_hists = self._tabulate_genes(res, names, small, lo) if self.annotated else None
        return (lo, hi, names, small, cs, gene_hists)

    def _tabulate_genes(self, res, names, small, first_contig: int = 0):
        """occupancy histogram of every gene's positions, summed per chromosome (index.py:1055-1064,
        1079-1082), from the rows in HBM: {chrom: (gene_count, hist[N+1])} in sorted-chr order"""
        genes = self.load_genes()
        out = {}
        for chrom, grp in genes.groupby("chr", sort=True):
            if chrom not in names:
                out[chrom] = (len(grp), np.zeros(self.ngenomes + 1, np.int64))
                continue
            ci = names.index(chrom)
            size = small[ci][3]["nkmers"]
            st, en = grp["start"].to_numpy(np.int64), grp["end"].to_numpy(np.int64)
            ok = (en > st) & (st >= 0) & (en <= size)
            for s_, e_ in zip(st[~ok], en[~ok]):
                self.log.warning(f"Skipping gene at {chrom}:{s_}-{e_}, coordinates out-of-bounds")
            hist = np.zeros(self.ngenomes + 1, np.int64)
            if ok.any():
                h, _ = res.window_stats(first_contig + ci, st[ok], en[ok], step=1, colsums=False)
                hist = h.sum(axis=0).astype(np.int64)
            out[chrom] = (len(grp), hist)
            self.log.info(f"Annotated {chrom}")
        return out

    def write_from_result(self, job, gi: int = 0, bgzf_threads: Optional[int] = None):
        """anchor/<name>/ exactly as the reference lays it out (cpp/anchor.cpp:37-109,
        index.py:1035-1094): this genome's contig range of the (possibly shared) result, the two
        bitmaps streamed from HBM by the library.  The caller closes the result."""
        res = job["res"]
        lo, hi, names, small, cs, gene_hists = job["genomes"][gi]
        os.makedirs(self.prefix, exist_ok=True)
        nthreads = bgzf_threads or self._bgzf_threads()
        for s in self.steps:
            gz, gzi = self.bitmap_gz_fname(s), self.bitmap_gzi_fname(s)
            res.write_bgzf(s, gz + ".tmp", gzi + ".tmp", level=self.index.bgzf_level, threads=nthreads, first_contig=lo,
                           ncontigs=hi - lo)
            os.replace(gz + ".tmp", gz)
            os.replace(gzi + ".tmp", gzi)
        self._write_tables(names, small, cs, gene_hists)
        self.close_log()

    def _bgzf_threads(self) -> int:
        return max(1, min(64, self.index.cores if self.index.cores > 1 else engine.usable_cpus()))

    def _write_tables(self, names, small: "engine.SmallOutputs", paircount_sums, gene_hists=None):
        """bitsum.bins.tsv, bitsum.genes.tsv, total_paircounts.csv and chrs.tsv of the contigs ``names``; ``small``: their
        small outputs as ``AnchorResult.contigs_small`` gives them (an engine.SmallOutputs, nothing else)"""
        N = self.ngenomes
        # the contigs' bins in one array: the text is formatted by the library (two million rows per anchor genome for
        # an assembly of 20 000 contigs; row by row in the interpreter that was most of such a run)
        small.write_bins_tsv(self.bins_fname, N)
        chr_rows: List[Tuple[str, int, int, int]] = [
            (chrom, ci, int(small.nkmers[ci]), gene_hists[chrom][0] if gene_hists and chrom in gene_hists else 0)
            for ci, chrom in enumerate(names)]
        if len(names) <= 1000:
            for chrom in names:
                self.log.info(f"Anchored {chrom}")
        else:  # (a log line per contig of a fragmented assembly is a second of logging per genome)
            self.log.info(f"Anchored {len(names)} contigs ({names[0]} ... {names[-1]})")
        if gene_hists is not None:  # bitsum.genes.tsv: one row per annotated chromosome (index.py:1079-1082)
            self._write_gene_sums(self.chr_genes_fname, gene_hists)
        # total_paircounts.csv (index.py:1068-1074): count[g] = positions holding genome g's bit
        counts = pd.Series(np.asarray(paircount_sums, dtype=np.int64), index=self.index.genome_names)
        pd.DataFrame({"count": counts, "frac": counts / counts[self.name]}).to_csv(
            os.path.join(self.prefix, "total_paircounts.csv"))
        chrs = pd.DataFrame(chr_rows, columns=["name", "id", "size", "gene_count"]).set_index("name")
        self.set_chrs(chrs)
        self.write_benchmark()
        self.chrs.to_csv(self.chrs_fname, sep="\t")  # written last: it is the rule's completion marker
        self.index._completed.append(self.name)

    def _write_gene_sums(self, path: str, gene_hists) -> None:
        pd.DataFrame([h for _, h in gene_hists.values()], index=pd.Index(list(gene_hists), name="chr"),
                     columns=range(self.ngenomes + 1)).to_csv(path, sep="\t")

    # ---- ANNOTATE: gene and annotation tracks of an anchored genome (index.py:615-651, 663-791, 971-1010) ----
    def tabix_fname(self, typ: str) -> str:
        return os.path.join(self.prefix, f"{typ}.bed.gz")

    def tabix_idx_fname(self, typ: str) -> str:
        return self.tabix_fname(typ) + ".csi"

    @property
    def anno_types_fname(self):
        return os.path.join(self.prefix, "anno_types.txt")

    annotate_budget = 8 << 30  # bitmap.1 payload bytes of one batch of chromosomes read back into HBM

    def run_annotate(self, gff=None, nogene=False) -> None:
        """Counterpart of ``Genome.run_annotate(gff_file, nogene=...)`` (index.py:971-1010): the GFF (default: the sample's
        own) -> anno.bed.gz(.csi) and anno_types.txt, and unless ``nogene``, per-gene occupancy from bitmap.1.gz inflated on
        the GPU -> gene.bed.gz(.csi), bitsum.genes.tsv and the ``gene_count`` column of chrs.tsv.  Every file is written to a
        temporary and renamed."""
        from . import annotation as an
        gff = self.gff if gff is None else gff
        if gff is None or (not isinstance(gff, str) and pd.isna(gff)):
            raise ValueError(f"{self.name}: no GFF to annotate with")
        idx = self.index
        genes, annos, types = an.gff_records(gff, idx.gff_gene_types, idx.gff_anno_types, idx.gff_name)
        an.write_track(self.tabix_fname("anno"), annos)
        self._write_text(self.anno_types_fname, "".join(f"{t}\n" for t in types))
        if nogene:
            return
        self.load_chrs()
        N = self.ngenomes
        occ = np.zeros((len(genes), N + 1), np.int64)  # each gene's own histogram (0 when skipped)
        gene_hists = {}
        grouped = {chrom: grp.index.to_numpy() for chrom, grp in genes.groupby("chr", sort=True)}
        work = []  # (chrom, gene rows, starts, ends) of the genes inside their chromosome
        for chrom, rows in grouped.items():
            gene_hists[chrom] = (len(rows), np.zeros(N + 1, np.int64))
            if chrom not in self.chrs.index:
                self.log.warning(f"Skipping {len(rows)} gene(s) on {chrom}: chromosome not found")
                logger.warning(f"{self.name}: skipping {len(rows)} gene(s) on {chrom}: chromosome not found")
                continue
            size = int(self.chrs.loc[chrom, "size"])
            st, en = genes.loc[rows, "start"].to_numpy(np.int64), genes.loc[rows, "end"].to_numpy(np.int64)
            ok = (en > st) & (st >= 0) & (en <= size)
            for s_, e_ in zip(st[~ok], en[~ok]):
                self.log.warning(f"Skipping gene at {chrom}:{s_}-{e_}, coordinates out-of-bounds")
            if ok.any():
                work.append((chrom, rows[ok], st[ok], en[ok]))
        for batch in self._annotate_batches([w[0] for w in work]):
            res = self._rows_from_disk(batch)
            try:
                for ci, chrom in enumerate(batch):
                    _, rows, st, en = next(w for w in work if w[0] == chrom)
                    h, _ = res.window_stats(ci, st, en, step=1, colsums=False)
                    occ[rows] = h.astype(np.int64)
                    gene_hists[chrom] = (gene_hists[chrom][0], occ[rows].sum(axis=0))
                    self.log.info(f"Annotated {chrom}")
            finally:
                res.close()
        an_genes = an.gene_track(genes, occ[:, 1], occ[:, N], N)
        an.write_track(self.tabix_fname("gene"), an_genes)
        self._write_gene_sums(self.chr_genes_fname + ".tmp", gene_hists)
        os.replace(self.chr_genes_fname + ".tmp", self.chr_genes_fname)
        counts = pd.Series({c: n for c, (n, _) in gene_hists.items()}, dtype=np.int64)
        self.chrs["gene_count"] = counts.reindex(self.chrs.index, fill_value=0).astype(np.int64).to_numpy()
        self.chrs.to_csv(self.chrs_fname + ".tmp", sep="\t")
        os.replace(self.chrs_fname + ".tmp", self.chrs_fname)

    @staticmethod
    def _write_text(path: str, text: str) -> None:
        with open(path + ".tmp", "w") as f:
            f.write(text)
        os.replace(path + ".tmp", path)

    def _annotate_batches(self, chroms: List[str], budget: Optional[int] = None) -> List[List[str]]:
        """runs of chromosomes that are neighbours in the file, each run's bitmap.1 rows within ``budget`` (default:
        annotate_budget; a longer chromosome is a run of its own).  bitmap.1 bytes whatever file is read: a rows container
        holds the full-resolution rows of its chromosomes even when only the low-resolution ones are filled"""
        budget = self.annotate_budget if budget is None else budget
        order = {c: i for i, c in enumerate(self.chrs.index)}
        chroms = sorted(chroms, key=order.get)
        nb = self.nbytes
        out, cur, cur_bytes = [], [], 0
        for c in chroms:
            b = int(self.chrs.loc[c, "size"]) * nb
            if cur and (order[c] != order[cur[-1]] + 1 or cur_bytes + b > budget):
                out.append(cur)
                cur, cur_bytes = [], 0
            cur.append(c)
            cur_bytes += b
        if cur:
            out.append(cur)
        return out

    def _rows_from_disk(self, chroms: List[str], step: int = 1) -> "engine.AnchorResult":
        """a rows result over consecutive chromosomes of chrs.tsv, filled from bitmap.<step>.gz (1 or the index's
        low-resolution step) on the GPU"""
        sizes = [int(self.chrs.loc[c, "size"]) for c in chroms]
        if step == 1:
            row0 = int(self.chrs["size"].cumsum().shift(fill_value=0).loc[chroms[0]])
        else:
            row0 = int(self.offsets.loc[chroms[0], step])
        return self._rows_container(sizes, step, row0)

    def _rows_container(self, nkmers: List[int], step: int, row0: int) -> "engine.AnchorResult":
        """a rows result over contigs of ``nkmers`` rows, filled on the GPU from bitmap.<step>.gz's payload from row ``row0``"""
        return engine.AnchorResult.from_bgzf(self.index.context, int(self.index.k), self.ngenomes, nkmers, self.bitmap_gz_fname(step),
                                             self.bitmap_gzi_fname(step), file_row0=row0, step=step,
                                             lowres_step=int(self.index.lowres_step))

    # ---- PLACE: a read set's column joined with this anchor's rows (pg_place.hip) ----
    place_budget = 8 << 30            # bitmap.1 bytes of one batch of chromosomes read back into HBM
    PLACE_MAX_POSITIONS = 1 << 30     # k-mer positions of one batch: the keys a count table holds

    def _place_batches(self, chroms: List[str]) -> List[List[str]]:
        """``_annotate_batches`` under ``place_budget``, each run cut further so that a batch has at most PLACE_MAX_POSITIONS k-mer
        positions and its count table (8-byte keys and one 4-byte plane per slot) and rows fit the free memory"""
        from .copies import table_slots
        free = self.index.context.mem_info()[0]
        nb = self.nbytes

        def cost(pos: int) -> int:
            return table_slots(pos) * 12 + pos * nb
        out = []
        for run in self._annotate_batches(chroms, self.place_budget):
            cur, pos = [], 0
            for c in run:
                p = int(self.chrs.loc[c, "size"])
                if cur and (pos + p > self.PLACE_MAX_POSITIONS or cost(pos + p) > 0.8 * free):
                    out.append(cur)
                    cur, pos = [], 0
                cur.append(c)
                pos += p
            if cur:
                out.append(cur)
        return out

    def place_counts(self, reads, chroms=None, bin_size: int = 100000, min_count: int = 2, batch_bytes: Optional[int] = None):
        """(bins, valid, held, col, both, stats) of the read set ``reads`` (FASTQ paths, plain or ``.gz``, four lines per record)
        along this anchor: ``bins`` = chrom, start, end of the bins of ``similarity_bin_geometry`` at step 1 over ``chroms`` (None:
        all, in chrs.tsv order), and per bin the valid rows, the rows whose k-mer the reads hold at least ``min_count`` times, and
        per genome of the index the rows with its bit and with both.  ``stats``: reads, read_bases, hits, depth_hist, depth_mode,
        min_count.  Per batch of chromosomes (``_place_batches``): the chromosomes packed from the FASTA, their k-mers into a count
        table of one plane, every FASTQ batch of ``batch_bytes`` text bytes joined on the GPU (``SeqSet.from_fastq``) and streamed
        through it, one depth profile of the anchor, the rows inflated from bitmap.1, one ``sample_agree`` over the bins.  THE READ
        FILES ARE READ AGAIN FOR EVERY BATCH OF CHROMOSOMES: packed reads are not kept."""
        from . import place as pl
        idx, ctx, k = self.index, self.index.context, int(self.index.k)
        bin_size, min_count = int(bin_size), int(min_count)
        if min_count < 1:
            raise ValueError(f"place: min_count must be at least 1, got {min_count}")
        if self.fasta is None or pd.isna(self.fasta) or is_fastq(self.fasta):
            raise ValueError(f"place: anchor {self.name!r} has no assembly FASTA ({self.fasta})")
        if not os.path.exists(self.bitmap_gz_fname(1)):
            raise ValueError(f"place: anchor {self.name!r} has no {os.path.basename(self.bitmap_gz_fname(1))}: it was not anchored")
        chroms = self._checked_chroms(1, bin_size, chroms=chroms)
        reads = [reads] if isinstance(reads, (str, os.PathLike)) else list(reads)
        for r in reads:
            if not os.path.isfile(r):
                raise ValueError(f"place: no read file {os.fspath(r)!r}")
        batch_bytes = pl.DEFAULT_BATCH_BYTES if batch_bytes is None else int(batch_bytes)
        N = self.ngenomes
        mine = self.name not in idx._seqsets
        ss = idx.seqset_for(self.name)
        frames, counts = [], []
        stats = {"reads": 0, "read_bases": 0, "hits": 0, "depth_hist": np.zeros(engine.COPIES_BINS, np.uint64), "min_count": min_count}
        try:
            # the FASTA's records are the chromosomes of chrs.tsv, in its order
            if len(ss.names) != len(self.chrs.index):
                raise ValueError(f"place: {self.fasta} holds {len(ss.names)} records, chrs.tsv {len(self.chrs.index)} chromosomes")
            for i, (c, size) in enumerate(zip(self.chrs.index, self.chrs["size"])):
                want = max(0, int(ss.lens[i]) - k + 1)
                if str(ss.names[i]) != str(c) or want != int(size):
                    raise ValueError(f"place: record {i} of {self.fasta} is {ss.names[i]!r} with {want} k-mers, chromosome {i} of "
                                     f"chrs.tsv is {c!r} with {int(size)}")
            order = {c: i for i, c in enumerate(self.chrs.index)}
            for bi, batch in enumerate(self._place_batches(chroms)):
                sizes = [int(self.chrs.loc[c, "size"]) for c in batch]
                geo = [self.similarity_bin_geometry(sz, 1, bin_size) for sz in sizes]
                if sum(sizes) == 0:
                    continue
                ass = engine.SeqSet.concat_ranges(ctx, [(ss, order[batch[0]], len(batch))])
                table = res = None
                try:
                    table = engine.CopyTable(ctx, k, sum(sizes), 1)
                    table.insert(ass)
                    for path in reads:
                        fb = pl.FastqBatches(path, batch_bytes)
                        for buf in fb:
                            rs, n, used = engine.SeqSet.from_fastq(ctx, buf)
                            try:
                                stats["hits"] += table.count(0, rs)
                                if bi == 0:
                                    stats["reads"] += n
                                    stats["read_bases"] += int(rs.lens[0]) - max(n - 1, 0)
                            finally:
                                rs.close()
                            fb.advance(used)
                    stats["depth_hist"] += table.profile(ass)[0][:, 0, :].sum(axis=0)
                    res = self._rows_from_disk(batch)
                    ci = np.concatenate([np.full(len(g[0]), i, np.uint32) for i, g in enumerate(geo)])
                    st = np.concatenate([g[1] for g in geo])
                    en = np.concatenate([g[2] for g in geo])
                    counts.append(table.sample_agree(0, min_count, ass, res, ci, st, en))
                finally:
                    if res is not None:
                        res.close()
                    if table is not None:
                        table.close()
                    ass.close()
                for c, sz, g in zip(batch, sizes, geo):
                    frames.append(pd.DataFrame({"chrom": c, "start": g[0] * bin_size, "end": np.minimum((g[0] + 1) * bin_size, sz)}))
        finally:
            if mine:
                idx.drop_seqset(self.name)
        bins = pd.concat(frames, ignore_index=True) if frames else pd.DataFrame({"chrom": [], "start": [], "end": []})
        cat = lambda j, shape: np.concatenate([c[j] for c in counts]) if counts else np.zeros(shape, np.uint64)
        stats["depth_mode"] = pl.depth_mode(stats["depth_hist"])
        return bins, cat(0, 0), cat(1, 0), cat(2, (0, N)), cat(3, (0, N)), stats

    # ---- INTROGRESSIONS: binned k-mer similarity (call_introgressions.py: bitmap_to_bins) ----
    # HBM of one batch of chromosomes read back: their bitmap.1 rows (the container holds them, and zeroes them, when the
    # low-resolution file is read too), so a batch takes at most this much, plus 1 / lowres_step of it, whatever the step
    similarity_budget = 8 << 30

    @staticmethod
    def similarity_bin_geometry(size: int, step: int, bin_size: int):
        """(bin numbers, first sampled row, end sampled row) of the bins of a chromosome of ``size`` positions sampled every
        ``step``: sampled row j is position j * step, bin b holds the rows with j * step // bin_size == b, and bins without a
        sampled row are left out"""
        n = -(-int(size) // int(step))  # len(range(0, size, step))
        if n == 0:
            return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
        b = np.arange((n - 1) * step // bin_size + 1, dtype=np.int64)
        s = -(-(b * bin_size) // step)
        e = np.minimum(n, -(-((b + 1) * bin_size) // step))
        ok = s < e
        return b[ok], s[ok], e[ok]

    def similarity_keep_words(self, keep) -> Optional[np.ndarray]:
        """genome names (or column numbers) -> the keep mask's 32-bit words; None for no mask"""
        if keep is None:
            return None
        names = list(self.index.genome_names)
        words = np.zeros((self.ngenomes + 31) // 32, np.uint32)
        for g in keep:
            i = names.index(g) if not isinstance(g, (int, np.integer)) else int(g)
            if not 0 <= i < self.ngenomes:
                raise ValueError(f"keep: genome {g!r} out of range")
            words[i // 32] |= np.uint32(1 << (i % 32))
        return words

    def _base_step(self, step: int) -> Tuple[int, int]:
        """(bstep, stride) of a sampling step: it reads every ``stride``-th row of bitmap.<bstep>.gz, the coarsest bitmap
        whose step divides it"""
        bstep = max(s for s in self.steps if step % s == 0)
        return bstep, step // bstep

    def _checked_chroms(self, step: int, bin_size: Optional[int] = None, region=None, chroms=None) -> List[str]:
        """The row readers' argument checks, in the order they refuse, and the chromosomes to visit: that of ``region`` =
        (chrom, start, end), or ``chroms`` as strings; every chromosome where that is None."""
        if bin_size is None and step < 1:
            raise ValueError(f"step must be positive, got {step}")
        if bin_size is not None and (step < 1 or bin_size < 1):
            raise ValueError(f"step and bin_size must be positive, got {step}, {bin_size}")
        if self.chrs is None:
            self.load_chrs()
        if region is not None:
            chrom, start, end = region
            if chrom is None and (start is not None or end is not None):
                raise ValueError("start and end need a chromosome")
            chroms = None if chrom is None else [chrom]
        elif chroms is not None:
            chroms = [str(c) for c in chroms]
        chroms = list(self.chrs.index) if chroms is None else chroms
        for c in chroms:
            if c not in self.chrs.index:
                raise KeyError(f"{self.name}: no chromosome {c!r}")
        return chroms

    def _binned_batches(self, chroms: List[str], step: int, bin_size: int, fn):
        """(geo, per): ``geo[c]`` = similarity_bin_geometry of chromosome c, ``per[c]`` = its bins' rows of what
        ``fn(res, ci, st, en, bstep, stride)`` gave — an array, or a tuple of arrays, with one leading row per bin — for the
        chromosomes that have bins.  One container and one ``fn`` call per batch of neighbouring chromosomes whose bitmap.1
        rows fit ``similarity_budget`` bytes of HBM; the container is closed before the next one is opened."""
        bstep, stride = self._base_step(step)
        geo = {c: self.similarity_bin_geometry(int(self.chrs.loc[c, "size"]), step, bin_size) for c in chroms}
        per = {}
        for batch in self._annotate_batches([c for c in dict.fromkeys(chroms) if len(geo[c][0])], self.similarity_budget):
            res = self._rows_from_disk(batch, bstep)
            try:
                ci = np.concatenate([np.full(len(geo[c][0]), i, np.uint32) for i, c in enumerate(batch)])
                st = np.concatenate([geo[c][1] for c in batch])
                en = np.concatenate([geo[c][2] for c in batch])
                got = fn(res, ci, st, en, bstep, stride)
            finally:
                res.close()
            at = 0
            for c in batch:
                nb = len(geo[c][0])
                per[c] = tuple(a[at:at + nb] for a in got) if isinstance(got, tuple) else got[at:at + nb]
                at += nb
        return geo, per

    def kmer_similarity_bins(self, chroms=None, step: int = 100, bin_size: int = 1_000_000, omit_fixed: bool = False,
                             keep=None) -> Dict[str, pd.DataFrame]:
        """{chrom: DataFrame} as ``bitmap_to_bins(genome.query(chrom, 0, size, step), bin_size, ...)`` of the reference's
        introgression caller gives it: one row per genome, one column per bin (its start position), each value the bin's
        column sum over the largest column sum of the bin.  ``keep`` (genome names): rows holding none of their bits get them
        (--rmu); ``omit_fixed``: rows holding every genome are dropped (--rmf).  A bin whose rows were all dropped is 1.0, a
        bin whose sums are all zero NaN.  The rows are read back from the bitmap on the GPU (batches of neighbouring
        chromosomes whose bitmap.1 rows fit ``similarity_budget`` bytes of HBM) and binned by k_bin_colsums, one launch per batch."""
        step, bin_size = int(step), int(bin_size)
        chroms = self._checked_chroms(step, bin_size, chroms=chroms)
        kw = self.similarity_keep_words(keep)
        names = pd.Index(self.index.genome_names)
        geo, sums = self._binned_batches(chroms, step, bin_size, lambda res, ci, st, en, bstep, stride: res.bin_colsums(
            ci, st, en, step=bstep, stride=stride, keep_words=kw, omit_fixed=omit_fixed))
        return {c: self._similarity_frame(*sums[c], geo[c][0] * bin_size, names) if c in sums else
                pd.DataFrame(np.zeros((self.ngenomes, 0)), index=names, columns=pd.Index([], dtype=np.int64)) for c in chroms}

    @staticmethod
    def _similarity_frame(cs: np.ndarray, kept: np.ndarray, starts: np.ndarray, names: pd.Index) -> pd.DataFrame:
        """bins x genomes sums -> the genomes x bins frame of bitmap_to_bins: a bin without rows left is all 1 (its
        reindex fill value), every bin divided by its largest sum (0 / 0: NaN)"""
        v = cs.astype(np.float64)
        v[kept == 0] = 1.0
        with np.errstate(invalid="ignore", divide="ignore"):
            v = v / v.max(axis=1, keepdims=True)
        return pd.DataFrame(v.T, index=names, columns=pd.Index(np.asarray(starts, np.int64)))

    # ---- TREE: pair counts of the genomes over a region (view.py:751-764: create_tree) ----
    def _rows_region(self, bstep: int, row0: int, nrows: int) -> "engine.AnchorResult":
        """a rows result of ONE pseudo-contig: rows [row0, row0 + nrows) of bitmap.<bstep>.gz's payload, inflated on the GPU"""
        # (a container derives its low-resolution rows from its contig's length: the shortest contig with nrows of them)
        nk = nrows if bstep == 1 else (nrows - 1) * bstep + 1
        return self._rows_container([nk], bstep, row0)

    def _region_rows(self, chrom: str, start, end, step: int):
        """(bstep, stride, first payload row, rows) of what ``query(chrom, start, end, step)`` reads: ``rows`` rows of
        bitmap.<bstep>.gz from ``first``, of which it keeps every ``stride``-th"""
        bstep, stride = self._base_step(step)
        start = 0 if start is None else int(start)
        end = self.seq_len(chrom) if end is None else int(end)
        row0 = int(self.offsets.loc[chrom, bstep]) + start // bstep
        file_rows = int(np.ceil(self.sizes / bstep).sum())  # (query reads to the payload's end at most)
        nrows = min((end - 1 - start) // bstep + 1, file_rows - row0) if end > start and start >= 0 else 0
        return bstep, stride, row0, max(0, nrows)

    def _region_pieces(self, chrom: str, start, end, step: int, fn) -> list:
        """[(first sampled row, sampled rows, fn(res, sampled rows, bstep, stride))] of the consecutive pieces of what
        ``query(chrom, start, end, step)`` reads, ``res`` the piece's rows container: one container per piece, closed before
        the next one is opened.  A piece takes at most similarity_budget bytes of HBM (a container of low-resolution rows
        holds, zeroed, the full-resolution rows they span) and starts at the first row of the region's sampling phase inside it."""
        bstep, stride, row0, nrows = self._region_rows(chrom, start, end, step)
        per = max(1, int(self.similarity_budget) // (self.nbytes * bstep))
        out = []
        for p0 in range(0, nrows, per):
            p1 = min(p0 + per, nrows)
            first = -(-p0 // stride) * stride
            if first >= p1:
                continue
            ns = (p1 - first - 1) // stride + 1
            res = self._rows_region(bstep, row0 + first, p1 - first)
            try:
                out.append((first // stride, ns, fn(res, ns, bstep, stride)))
            finally:
                res.close()
        return out

    def _pair_counts(self, chrom=None, start=None, end=None, step: int = 1):
        """(N x N int64 pair counts, sampled rows they were taken over)"""
        step = int(step)
        chroms = self._checked_chroms(step, region=(chrom, start, end))
        N = self.ngenomes
        total, seen = np.zeros((N, N), np.int64), 0
        for c in chroms:
            for _, ns, counts in self._region_pieces(c, start, end, step, lambda res, ns, bstep, stride: res.pair_counts(
                    [0], [0], [ns], step=bstep, stride=stride)[0].astype(np.int64)):
                total += counts
                seen += ns
        return total, seen

    def pair_counts(self, chrom=None, start=None, end=None, step: int = 1) -> pd.DataFrame:
        """N x N integers, indexed and labelled by the genome names: entry (a, b) = rows of ``query(chrom, start, end, step)``
        holding both genomes' bits (``B.T @ B`` of that frame) — every such row, none of them read back to the host: the
        region's rows are inflated into HBM and reduced by k_pair_counts, in consecutive pieces of at most
        ``similarity_budget`` bytes.  ``chrom=None``: the sum over all chromosomes.  The diagonal are the column sums."""
        total, _ = self._pair_counts(chrom, start, end, step)
        names = pd.Index(self.index.genome_names)
        return pd.DataFrame(total, index=names, columns=names)

    # ---- FIND: runs of rows that these genomes hold and those lack (scripts/query_index.py: the "custom" query) ----
    def find_pattern(self, have, lack=(), min_have=None, max_lack=0, chrom=None, start=None, end=None, step: int = 1,
                     min_len: int = 1, max_gap: int = 0) -> pd.DataFrame:
        """chr, start, end, rows: the runs of consecutive rows of ``query(chrom, start, end, step)`` that MATCH — at least
        ``min_have`` of the ``have`` genomes (names or columns; default: all of them) hold the row's k-mer and at most
        ``max_lack`` of the ``lack`` genomes do.  ``start`` is the label ``query`` gives the run's first row, ``end`` the label
        of its last row + 1.  Runs separated by at most ``max_gap`` non-matching rows are merged, then spans shorter than
        ``min_len`` rows dropped; ``rows`` = the matching rows inside the span.  ``chrom=None``: every chromosome, and no run
        joins two of them.  The rows are inflated into HBM in consecutive pieces of at most ``similarity_budget`` bytes and
        searched there by k_find_runs; only the runs come back."""
        from . import find
        step = int(step)
        chroms = self._checked_chroms(step, region=(chrom, start, end))
        hw, lw, min_have, max_lack = find.rule_words(self.index.genome_names, have, lack, min_have, max_lack)
        find.merge_runs([], [], min_len, max_gap)  # (its argument checks, before anything is read)

        def runs_of(res, ns, bstep, stride):
            runs, _ = res.find_runs([0], [0], [ns], hw, lw, min_have, max_lack, step=bstep, stride=stride)
            return runs[:, 1], runs[:, 2]
        frames = []
        for c in chroms:
            pieces = [(j0, ns, a, b) for j0, ns, (a, b) in self._region_pieces(c, start, end, step, runs_of)]
            s, e, rows = find.merge_runs(*find.join_pieces(pieces), min_len, max_gap)
            label0 = 0 if start is None else int(start)  # (query labels its j-th row start + j * step)
            frames.append(pd.DataFrame({"chr": np.full(len(s), c, object), "start": label0 + s * step,
                                        "end": label0 + (e - 1) * step + 1, "rows": rows}))
        return pd.concat(frames, ignore_index=True)

    def pattern_density(self, have, lack=(), min_have=None, max_lack=0, chroms=None, step: int = 1,
                        bin_size: int = 1_000_000) -> pd.DataFrame:
        """chr, start, matched, rows: per bin of ``bin_size`` positions of every chromosome (bins and batches of chromosomes as
        ``kmer_similarity_bins`` takes them), the rows sampled every ``step`` that match the rule of ``find_pattern`` and the
        sampled rows of the bin.  One k_find_runs count launch per batch; no run is written."""
        from . import find
        step, bin_size = int(step), int(bin_size)
        chroms = self._checked_chroms(step, bin_size, chroms=chroms)
        hw, lw, min_have, max_lack = find.rule_words(self.index.genome_names, have, lack, min_have, max_lack)
        geo, matched = self._binned_batches(chroms, step, bin_size, lambda res, ci, st, en, bstep, stride: res.find_counts(
            ci, st, en, hw, lw, min_have, max_lack, step=bstep, stride=stride)[1].astype(np.int64))
        frames = [pd.DataFrame({"chr": np.full(len(geo[c][0]), c, object), "start": geo[c][0] * bin_size,
                                "matched": matched.get(c, np.zeros(0, np.int64)), "rows": geo[c][2] - geo[c][1]}) for c in chroms]
        return pd.concat(frames, ignore_index=True) if frames else pd.DataFrame(
            {"chr": np.zeros(0, object), "start": np.zeros(0, np.int64), "matched": np.zeros(0, np.int64), "rows": np.zeros(0, np.int64)})

    # ---- PATTERNS: which presence/absence patterns occur, and how many rows each holds (query + value_counts) ----
    def pattern_counts(self, genomes=None, chrom=None, start=None, end=None, step: int = 1):
        """(keys uint64, counts uint64, selected names): the pattern spectrum of the rows of ``query(chrom, start, end, step)``
        over the ``genomes`` selected (names or columns, at most 64; default: all of them) — bit i of a key is the row's bit
        for the i-th selected genome in column order, ``keys`` ascending.  ``chrom=None``: every chromosome.  The rows are
        inflated into HBM in consecutive pieces of at most ``similarity_budget`` bytes and reduced there by k_pattern_counts,
        one call per piece; pieces and chromosomes are added up on the host.  No row comes back."""
        from . import patterns
        step = int(step)
        chroms = self._checked_chroms(step, region=(chrom, start, end))
        words, selected = patterns.select_words(self.index.genome_names, genomes)
        parts = []
        for c in chroms:
            parts += [kc for _, _, kc in self._region_pieces(c, start, end, step, lambda res, ns, bstep, stride: res.pattern_counts(
                [0], [0], [ns], words, step=bstep, stride=stride))]
        keys, counts = patterns.merge(parts)
        return keys, counts, selected

    def pattern_spectrum(self, genomes=None, chrom=None, start=None, end=None, step: int = 1, top: Optional[int] = None,
                         min_rows: int = 1) -> pd.DataFrame:
        """pattern, n, rows, frac: the presence/absence patterns that occur in the rows of ``query(chrom, start, end, step)``
        and the rows each holds — ``value_counts()`` of that frame's ``genomes`` columns, none of it read back to the host
        (``pattern_counts``).  ``pattern`` has one 0 / 1 per selected genome in column order, ``n`` counts its ones, ``frac`` is
        rows over all rows of the region; sorted by rows descending, then pattern.  ``min_rows`` drops rarer patterns, ``top``
        keeps the first so many (``patterns.spectrum_frame``)."""
        from . import patterns
        patterns.spectrum_frame([], [], ["-"], top, min_rows)  # (its argument checks, before anything is read)
        keys, counts, selected = self.pattern_counts(genomes, chrom, start, end, step)
        return patterns.spectrum_frame(keys, counts, selected, top, min_rows)

    # ---- GAPS: per genome, the runs of rows it lacks — where and how it differs from this anchor ----
    def _absence(self, genomes, chrom, start, end, step: int, maxlen: int, min_len: int, max_len: int, emit: bool = True):
        """([(chrom, sampled rows, runs, hist, absent, edges)], selected names): ``gaps.join_pieces`` of every chromosome of
        the region.  The rows are inflated into HBM in consecutive pieces of at most ``similarity_budget`` bytes, each reduced
        by one k_absence_runs call; runs are joined across the pieces' borders on the host."""
        from . import gaps
        chroms = self._checked_chroms(step, region=(chrom, start, end))
        gaps.check_lengths(maxlen, min_len, max_len)
        words, selected = gaps.select_words(self.index.genome_names, genomes)

        def reduce(res, ns, bstep, stride):
            runs, hist, absent, edges = res.absence_runs([0], [0], [ns], words, maxlen, min_len, max_len, step=bstep, stride=stride,
                                                         emit=emit)
            return runs[:, 1:], hist[0], absent[0], edges[0]
        out = []
        for c in chroms:
            pieces = [(j0, ns) + got for j0, ns, got in self._region_pieces(c, start, end, step, reduce)]
            out.append((c, sum(ns for _, ns, *_ in pieces)) + gaps.join_pieces(pieces, self.ngenomes, maxlen, min_len, max_len))
        return out, selected

    def _absence_frames(self, parts, selected, start, step: int, runs: bool = True):
        """(runs frame, summed hist, summed absent, summed rows of open runs, sampled rows) of ``_absence``'s parts"""
        from . import gaps
        names, k = np.array(self.index.genome_names, object), int(self.index.k)
        label0 = 0 if start is None else int(start)  # (query labels its j-th row start + j * step)
        frames = []
        hist = absent = open_rows = 0
        nrows = 0
        for c, ns, r, h, a, edges in parts:
            hist, absent, open_rows, nrows = hist + h, absent + a, open_rows + gaps.open_rows(edges, ns), nrows + ns
            if not runs:
                continue
            r = r[np.lexsort((r[:, 0], r[:, 1]))]  # by position, then genome
            first = label0 + r[:, 1] * step
            if step == 1:
                cls, site, _ = gaps.classify(r[:, 2], k, first)
            else:
                cls, site = np.full(len(r), "", object), np.full(len(r), -1, np.int64)
            frames.append(pd.DataFrame({"chr": np.full(len(r), c, object), "start": first, "end": label0 + (r[:, 1] + r[:, 2] - 1) * step + 1,
                                        "genome": names[r[:, 0]], "rows": r[:, 2], "class": cls, "site": site}))
        frame = pd.concat(frames, ignore_index=True) if frames else pd.DataFrame(
            {"chr": np.zeros(0, object), "start": np.zeros(0, np.int64), "end": np.zeros(0, np.int64), "genome": np.zeros(0, object),
             "rows": np.zeros(0, np.int64), "class": np.zeros(0, object), "site": np.zeros(0, np.int64)})
        return frame, hist, absent, open_rows, nrows

    def absence_runs(self, genomes=None, chrom=None, start=None, end=None, step: int = 1, min_len: int = 1,
                     max_len: int = 0) -> pd.DataFrame:
        """chr, start, end, genome, rows, class, site: per genome of ``genomes`` (names or columns; default: all), the CLOSED
        runs of consecutive rows of ``query(chrom, start, end, step)`` that lack the genome's bit — a present row of the region
        on both sides — with min_len <= rows (and rows <= max_len unless that is 0); the two runs a genome may have at the
        region's edges are not listed.  ``start`` is the label ``query`` gives the run's first row, ``end`` the label of its
        last row + 1, as ``find_pattern``'s.  At step 1 ``class`` and ``site`` are ``gaps.classify``'s candidate class and
        anchor base of the run; at other steps "" and -1.  Sorted by chromosome, start, genome column.  ``chrom=None``: every
        chromosome, and no run joins two of them.  Every row is read once on the GPU for all genomes (k_absence_runs), in
        pieces of at most ``similarity_budget`` bytes; a run is never cut at a piece border."""
        step = int(step)
        parts, selected = self._absence(genomes, chrom, start, end, step, 1, min_len, max_len)
        return self._absence_frames(parts, selected, start, step)[0]

    def absence_spectrum(self, genomes=None, chrom=None, start=None, end=None, step: int = 1, maxlen: Optional[int] = None) -> pd.DataFrame:
        """genome, rows, runs: how many closed runs of each length every genome of ``genomes`` has in the rows of
        ``query(chrom, start, end, step)``; the bin ``rows`` = ``maxlen`` (default 4 k) holds the runs of maxlen rows and
        more (``gaps.spectrum_frame``).  No run is written."""
        return self.absence_tables(genomes, chrom, start, end, step, maxlen=maxlen, runs=False)[1]

    def absence_tables(self, genomes=None, chrom=None, start=None, end=None, step: int = 1, min_len: int = 1, max_len: int = 0,
                       maxlen: Optional[int] = None, runs: bool = True):
        """(``absence_runs``' frame, ``absence_spectrum``'s frame, ``gaps.summary_frame`` per genome — None unless step is 1
        and maxlen > k) from ONE pass over the region's rows; ``runs=False``: no run is written, the first frame is empty"""
        from . import gaps
        step, k = int(step), int(self.index.k)
        maxlen = 4 * k if maxlen is None else int(maxlen)
        parts, selected = self._absence(genomes, chrom, start, end, step, maxlen, min_len, max_len, emit=runs)
        frame, hist, absent, open_rows, nrows = self._absence_frames(parts, selected, start, step, runs)
        names = list(self.index.genome_names)
        cols = [names.index(g) for g in selected]
        spectrum = gaps.spectrum_frame(hist[cols], selected)
        summary = gaps.summary_frame(hist[cols], absent[cols], open_rows[cols], nrows, selected, k) if step == 1 and maxlen > k else None
        return frame, spectrum, summary

    # ---- UMAPS: chrom_umaps.csv and genome_umap.csv (index.py:1100-1167) ----
    @property
    def chrom_umaps_filename(self):
        return os.path.join(self.prefix, "chrom_umaps.csv")

    @property
    def genome_umap_filename(self):
        return os.path.join(self.prefix, "genome_umap.csv")

    def write_umaps(self) -> Tuple[str, str]:
        """Write ``chrom_umaps.csv`` — every chromosome's bins of ``chrom_umap.bin_size`` embedded on their own, ``chrom``
        as the index — and ``genome_umap.csv`` — all bins of ``genome_umap.bin_size`` in one embedding, no index — both with
        the columns chrom, start, end, umap1, umap2, cluster (index.py:1107-1129).  The bins' pair-count rows come from
        ``kmer_similarity_bins``; their exact nearest neighbours from k_knn_rows, all chromosomes in ONE segmented launch;
        graph, layout and clusters from ``umap.py`` on the host (its docstring says what is claimed of them)."""
        from . import umap
        ix = self.index
        if self.chrs is None:
            self.load_chrs()
        cu, gu = ix.chrom_umap, ix.genome_umap
        frame, X = umap.paircount_matrix(self, cu.bin_size)
        c = frame["chrom"].to_numpy()
        seg = np.concatenate([[0], np.flatnonzero(c[1:] != c[:-1]) + 1, [len(c)]]).astype(np.int64)  # (a chromosome's bins are consecutive rows)
        k = min(int(cu.neighbors), int(np.diff(seg).max()) - 1)
        idx = d2 = None
        if k >= 2:
            idx, d2 = engine.knn_rows(ix.context, X, k, seg)
        parts = []
        for lo, hi in zip(seg[:-1], seg[1:]):
            knn = None if idx is None else (idx[lo:hi] - np.int32(lo), d2[lo:hi])
            parts.append(umap.run_umap(X[lo:hi], frame.iloc[lo:hi], cu, knn=knn, name=self.name))
        self.chrom_umaps = (pd.concat(parts) if parts else pd.DataFrame(columns=umap.COLUMNS)).set_index("chrom")
        ix._write_atomically(self.chrom_umaps_filename, lambda tmp: self.chrom_umaps.to_csv(tmp))
        if int(gu.bin_size) != int(cu.bin_size):
            frame, X = umap.paircount_matrix(self, gu.bin_size)
        self.genome_umap = umap.run_umap(X, frame, gu, ctx=ix.context, name=self.name)
        ix._write_atomically(self.genome_umap_filename, lambda tmp: self.genome_umap.to_csv(tmp, index=False))
        return self.chrom_umaps_filename, self.genome_umap_filename

    def load_umaps(self) -> None:
        """``chrom_umaps`` (indexed by chrom) and ``genome_umap`` as the viewer reads them (index.py:1158-1167); None where the
        file is missing"""
        self.chrom_umaps = (pd.read_csv(self.chrom_umaps_filename, index_col="chrom")
                            if os.path.exists(self.chrom_umaps_filename) else None)
        self.genome_umap = pd.read_csv(self.genome_umap_filename) if os.path.exists(self.genome_umap_filename) else None

    def _tabix(self, typ: str):
        from . import annotation as an
        cache = self.__dict__.setdefault("_tabix_cache", {})
        if typ not in cache:
            path = self.tabix_fname(typ)
            cache[typ] = an.TabixTrack(path) if os.path.exists(path) else None
        return cache[typ]

    def query_genes(self, chrom=None, start=None, end=None) -> pd.DataFrame:
        from . import annotation as an
        cols = an.GENE_COLS + [1, self.ngenomes]
        tbx = self._tabix("gene")
        rows = tbx.fetch(chrom, start, end) if tbx is not None else []
        types = {"start": int, "end": int, 1: int, self.ngenomes: int}
        return pd.DataFrame(rows, columns=cols).astype(types)

    def query_anno(self, chrom, start, end) -> pd.DataFrame:
        from . import annotation as an
        tbx = self._tabix("anno")
        if tbx is None:
            return pd.DataFrame(columns=an.TABIX_COLS)
        df = pd.DataFrame(tbx.fetch(chrom, start, end), columns=an.TABIX_COLS).astype(an.TABIX_TYPES)
        df["type_id"] = self.anno_type_ids[df["type"]].to_numpy()
        return df

    @property
    def anno_type_ids(self) -> pd.Series:
        """type -> id as the viewer numbers them (index.py:705-727): ``exon`` first (id 0) when present, else from 1"""
        with open(self.anno_types_fname) as f:
            types = [t.strip() for t in f if t.strip()]
        if "exon" in types:
            types = ["exon"] + [t for t in types if t != "exon"]
        id0 = 0 if "exon" in types else 1
        return pd.Series({t: id0 + i for i, t in enumerate(types)}, dtype=np.int64)

    def run_anchor(self, table: engine.PanTable, logfile: Optional[str] = None, bgzf_threads: Optional[int] = None):
        """Counterpart of ``Genome.run_anchor(bitvecs, logfile)`` (index.py:1012-1097) and of
        ``KMCdb::anchor_fasta`` (cpp/anchor.cpp:37-109): walks the anchor FASTA, anchors every
        contig on the GPU and writes the anchor/<name>/ files.  ``table`` is the GPU-resident
        pan-kmer table standing in for the list of ``kmc/bitvec{i}`` prefixes."""
        self.setup_log(logfile)
        if not self.anchored:
            logger.info(f"Skipping non-anchor genome '{self.name}'")
            return
        ss = self.index.seqset_for(self.name)
        job = None
        try:
            job = self.anchor_on_gpu(table, ss)
            self.write_from_result(job, 0, bgzf_threads)
        finally:
            if job is not None:
                job["res"].close()
            self.index.drop_seqset(self.name)

    # ---- READ: what `panagram view` does with our files (index.py:615-658, 793-845) ----
    def init_read(self):
        if self.chrs is None:
            self.load_chrs()
        self.blocks = {s: load_bgz_blocks(self.bitmap_gzi_fname(s)) for s in self.steps}
        self.bitsum_bins = pd.read_table(self.bins_fname)
        self.total_paircounts = pd.read_csv(os.path.join(self.prefix, "total_paircounts.csv"), index_col="name")

    def seq_len(self, seq_name):
        return int(self.sizes.loc[seq_name])

    def _bytes_to_bits(self, pac):
        return np.unpackbits(pac, bitorder="little", axis=1)[:, : self.ngenomes]

    def _query_bytes(self, name, start, end, step, bstep):
        byte_start = self.nbytes * (int(self.offsets.loc[name, bstep]) + (start // bstep))
        length = int((end - start) // bstep) + 1
        step = step // bstep
        buf = bgzf_read(self.bitmap_gz_fname(bstep), self.blocks[bstep], byte_start, length * self.nbytes)
        pac = np.frombuffer(buf, "uint8").reshape((len(buf) // self.nbytes, self.nbytes))
        return pac[::step] if step > 1 else pac

    def query(self, name, start=None, end=None, step=1) -> pd.DataFrame:
        if self.blocks is None:
            self.init_read()
        bstep, _ = self._base_step(step)
        start = 0 if start is None else start
        end = self.seq_len(name) if end is None else end
        pac = self._query_bytes(name, start, end - 1, step, bstep)
        bits = self._bytes_to_bits(pac)
        return pd.DataFrame(bits, index=pd.RangeIndex(start, end, step)[: len(bits)], columns=self.index.genome_names)


# ---------------------------------------------------------------------------
# process-level seam: `run_anchor <ngenomes> <root> [<name> <fasta>]...` (cpp/anchor.cpp:204-233)
# ---------------------------------------------------------------------------
def run_anchor_cli(argv: Sequence[str], device: int = 0) -> int:
    """Same argv and file contract as the reference's ``cpp/run_anchor`` binary: reads
    ``root/kmc/bitvec{i}`` (KMC1 or KMC2 layout, memory-mapped and imported on the GPU), writes
    ``root/anchor/<name>/{bitmap.1,bitmap.100}.gz(.gzi)``, ``bitsum.bins.tsv``, ``chrs.tsv``.  The reference runs
    its anchors as concurrent OpenMP iterations (cpp/anchor.cpp:217-223); here they share co-scheduled launches
    (batches bounded by the HBM their rows take) and their bitmaps are compressed on the GPU and streamed to the
    files by writer threads — the rows never visit the host uncompressed.  Unlike the reference, a missing or
    ill-formed DB is an error (cpp/anchor.cpp:29 ignores OpenForRA's result)."""
    from concurrent.futures import ThreadPoolExecutor
    ngenomes = int(argv[0])
    root = argv[1]
    pairs = argv[2:]
    if len(pairs) > 2 * ngenomes:
        print(f"Error: expected {ngenomes * 2 + 1} or fewer arguments")
        return 1
    ndbs = (ngenomes + 31) // 32
    ctx = engine.Context(device)
    prefixes = [os.path.join(root, "kmc", f"bitvec{i}") for i in range(ndbs)]
    k = engine.kmc_kmer_length(np.memmap(prefixes[0] + ".kmc_pre", dtype=np.uint8, mode="r"))
    anchors = list(zip(pairs[0::2], pairs[1::2]))
    # (how the table will be probed decides its minimizer window with the key count: one FASTA has no co-scheduling partner)
    tbl = engine.PanTable(ctx, k, ngenomes, coscheduled=max(1, len(anchors)))
    for i, p in enumerate(prefixes):
        tbl.load_kmc_files(i, p)
    nb_row = (ngenomes + 7) // 8
    bgzf_level = int(os.environ.get("PG_BGZF_LEVEL", "-2"))

    def write_anchor(res, name, lo, names):
        adir = os.path.join(root, "anchor", name)
        os.makedirs(adir, exist_ok=True)
        for step in (1, 100):
            res.write_bgzf(step, os.path.join(adir, f"bitmap.{step}.gz"), os.path.join(adir, f"bitmap.{step}.gzi"),
                           level=bgzf_level, threads=max(1, engine.usable_cpus() // 2), first_contig=lo, ncontigs=len(names))
        small = res.contigs_small(lo, len(names))  # (one call for all contigs; the bins' text is formatted by the library)
        small.write_bins_tsv(os.path.join(adir, "bitsum.bins.tsv"), ngenomes)
        with open(os.path.join(adir, "chrs.tsv"), "w") as fc:
            fc.write("name\tid\tsize\tgene_count\n" + "".join(f"{chrom}\t{ci}\t{int(small.nkmers[ci])}\t0\n" for ci, chrom in enumerate(names)))

    free = ctx.mem_info()[0]
    batch_bytes = int(min(Index.batch_bytes, max(1 << 30, (free - (6 << 30)) / 2.3)))
    with ThreadPoolExecutor(max_workers=2) as pool:
        previous = None  # (result, merged seqset, seqsets, futures) of the batch being written
        i = 0
        while i < len(anchors):
            batch, sets, rows = [], [], 0
            while i < len(anchors):
                name, fasta = anchors[i]
                ss = engine.SeqSet.from_fasta(ctx, fasta)
                need = int(ss.lens.sum()) * nb_row
                if batch and rows + need > batch_bytes:
                    ss.close()
                    break
                print(f"Anchoring {name} {fasta}")
                batch.append(name)
                sets.append(ss)
                rows += need
                i += 1
            merged = engine.SeqSet.concat(ctx, sets) if len(sets) > 1 else sets[0]
            res = engine.AnchorResult(tbl, merged, colsums=False)
            if len(sets) > 1:
                res.coschedule(np.repeat(np.arange(len(sets)), [len(x.names) for x in sets]),
                               contig_class=engine.homology_classes([x.names for x in sets]))
            res.run()
            first = np.cumsum([0] + [len(x.names) for x in sets])
            futs = [pool.submit(write_anchor, res, nm, int(first[j]), list(sets[j].names)) for j, nm in enumerate(batch)]
            if previous is not None:
                _join_cli_batch(*previous)
            previous = (res, merged if len(sets) > 1 else None, sets, futs)
        if previous is not None:
            _join_cli_batch(*previous)
    tbl.close()
    ctx.close()
    return 0


def _join_cli_batch(res, merged, sets, futs):
    try:
        for f in futs:
            f.result()
    finally:
        res.close()
        if merged is not None:
            merged.close()
        for x in sets:
            x.close()
