"""Thin object layer over the C-ABI: Context, PanTable, SeqSet, AnchorResult, BgzfWriter.

All compute happens in libpanagram_hip.so on the GPU; this file moves pointers.
numpy arrays are the host buffers the ABI asks the caller to own.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
import weakref
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import PG_ANCHOR_COLSUMS, PG_ANCHOR_COLUMNS_ONLY, PG_ANCHOR_ROWS_ONLY, PanagramHipError, check  # noqa: F401


def usable_cpus() -> int:
    """Host cores this process may actually use: the scheduler affinity, capped by the cgroup CPU
    quota (a container can see 256 hardware threads and be allowed 16 cores' worth of time)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, n)


def kmc_kmer_length(pre) -> int:
    """k of a KMC database from the image of its .kmc_pre file (either layout)"""
    v = _bytes_view(pre)
    k = C.c_uint32()
    check(_lib.load().pg_kmc_kmer_length(_ptr(v), v.size, C.byref(k)))
    return int(k.value)


# k_probe can emit a one-genome block's bit columns itself (ROWMODE 3: no row buffer at all).  Off by default: since the
# probe's round-2 diet the rows + k_cols_extract_b1 route is the faster one (one GPU as rank 0 of 8, 8 x 10^8 positions:
# 6.50 ms per step against 7.15, tools/ab_sharded.sh); PG_COLUMNS_DIRECT=1 turns it on where the row buffer's HBM matters.
COLUMNS_DIRECT = os.environ.get("PG_COLUMNS_DIRECT", "0") not in ("", "0")


_ADOPT_LOCK = threading.Lock()

# pattern runs (pg_find.hip).  FIND_CHUNK: sampled rows per workgroup — pg_kernels.h's constant, restated for the tests that aim
# at chunk edges (tests/test_find_cpu.py holds the two together); FIND_FIRST_CAP: runs AnchorResult.find_runs makes room for in
# its first call — 512 KiB of sampled row numbers; a second call with the exact total follows only beyond it
FIND_CHUNK = 4096
FIND_FIRST_CAP = 1 << 16

# pattern spectrum (pg_patterns.hip).  PATTERN_CHUNK: sampled rows per workgroup — pg_kernels.h's constant, restated for the tests
# that aim at chunk edges (tests/test_patterns_cpu.py holds the two together); PATTERN_FIRST_CAP: distinct patterns
# AnchorResult.pattern_counts makes room for in its first call — a table of 2 MiB in HBM; on "exceeded" the room grows 16-fold
# per call up to PATTERN_MAX_CAP (a table of 2 GiB)
PATTERN_CHUNK = 8192
PATTERN_FIRST_CAP = 1 << 16
PATTERN_MAX_CAP = 1 << 26

# absence runs (pg_gaps.hip).  GAPS_CHUNK: sampled rows per workgroup — pg_kernels.h's constant, restated for the tests that aim at
# chunk edges (tests/test_gaps_cpu.py holds the two together); GAPS_FIRST_CAP: runs AnchorResult.absence_runs makes room for in
# its first call
GAPS_CHUNK = 4096
GAPS_FIRST_CAP = 1 << 16

# presence profile (pg_profile.hip).  PROFILE_CHUNK: rows per workgroup — pg_kernels.h's constant, restated for the tests that aim
# at chunk edges (tests/test_search_cpu.py holds the two together)
PROFILE_CHUNK = 4096
PROFILE_MAX_GENOMES = 512  # columns k_presence_profile and k_sample_agree follow (tests/test_place_cpu.py holds it to the header)


def tile_positions() -> int:
    """k-mer positions per tile (launch unit; a bit-column block holds tile_positions() // 8 bytes per tile and genome:
    size buffers with AnchorResult.columns_bytes, never with a constant)"""
    return int(_lib.load().pg_tile_positions())


class _Owner:
    """Handles are destroyed children first (the C-ABI's rule): a parent remembers its live
    children weakly and closes them before itself, so that garbage collection — which finalises
    a dropped object graph in no particular order — can never free a table under a result."""

    def _adopt(self, child) -> None:
        with _ADOPT_LOCK:  # (sequence sets are parsed by several host threads at once: Index.load_inputs)
            if not hasattr(self, "_children"):
                self._children = []
            self._children = [w for w in self._children if w() is not None]
            self._children.append(weakref.ref(child))

    def _close_children(self) -> None:
        for w in getattr(self, "_children", []):
            c = w()
            if c is not None:
                c.close()
        self._children = []


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _bytes_view(seq) -> np.ndarray:
    """bytes / bytearray / str / uint8 ndarray -> contiguous uint8 ndarray (no copy when possible)."""
    if isinstance(seq, str):
        seq = seq.encode("latin-1")
    if isinstance(seq, np.ndarray):
        return np.ascontiguousarray(seq, dtype=np.uint8)
    return np.frombuffer(seq, dtype=np.uint8)


class Context(_Owner):
    """One per GPU / per rank."""

    def __init__(self, device: int = 0):
        self._lib = _lib.load()
        h = C.c_void_p()
        check(self._lib.pg_ctx_create(device, C.byref(h)))
        self._h = h
        self.device = device

    def set_stream(self, hip_stream: Optional[int]) -> None:
        """Adopt an external hipStream_t handle (0 = HIP's default stream, i.e. torch's
        default stream); ``None`` goes back to the context's own stream."""
        if hip_stream is None:
            check(self._lib.pg_ctx_set_stream(self._h, None, 1))
        else:
            check(self._lib.pg_ctx_set_stream(self._h, C.c_void_p(hip_stream), 0))

    def synchronize(self) -> None:
        check(self._lib.pg_ctx_synchronize(self._h))

    def mem_info(self) -> Tuple[int, int]:
        """(free, total) device memory in bytes"""
        f, t = C.c_uint64(), C.c_uint64()
        check(self._lib.pg_ctx_mem_info(self._h, C.byref(f), C.byref(t)))
        return int(f.value), int(t.value)

    def trim(self) -> None:
        """give back device memory kept for reuse (row buffers of closed results)"""
        check(self._lib.pg_ctx_trim(self._h))

    def host_buffer(self, nbytes: int) -> "HostBuffer":
        """page-locked host memory (pg_host_alloc): a numpy uint8 array that goes to the device by DMA"""
        return HostBuffer(self, nbytes)

    def torch_device(self):
        """the torch device the context's buffers live on (torch only carries the collectives' buffers)"""
        import torch
        return torch.device("cuda", self.device)

    def close(self) -> None:
        if self._h:
            self._close_children()
            self._lib.pg_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceBuffer:
    """a plain (zeroed) device buffer of the library's own — what the single-process genome-sharded pipeline exchanges
    its bit columns through (several ranks use torch tensors: the collective takes those)"""

    def __init__(self, ctx: Context, nbytes: int):
        self.ctx, self._lib, self.nbytes = ctx, ctx._lib, int(nbytes)
        p = C.c_void_p()
        check(self._lib.pg_device_alloc(ctx._h, self.nbytes, C.byref(p)))
        self._p = p

    def data_ptr(self) -> int:
        return int(self._p.value)

    def zero(self, nbytes: Optional[int] = None) -> None:
        check(self._lib.pg_device_memset(self.ctx._h, self._p, 0, self.nbytes if nbytes is None else nbytes))

    def close(self) -> None:
        if self._p:
            self._lib.pg_device_free(self.ctx._h, self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostBuffer:
    """``nbytes`` of page-locked host memory as ``.array`` (numpy uint8); ``close()`` gives it back (not before every view of
    ``.array`` is out of use)."""

    def __init__(self, ctx: Context, nbytes: int):
        import threading
        self.ctx, self.nbytes = ctx, int(nbytes)
        self._lock = threading.Lock()  # (a pool may give its buffers back from a helper thread while the context is being closed)
        p = C.c_void_p()
        check(ctx._lib.pg_host_alloc(ctx._h, self.nbytes, C.byref(p)))
        self._p = p
        self.array = np.ctypeslib.as_array((C.c_uint8 * max(1, self.nbytes)).from_address(p.value))[:self.nbytes]
        ctx._adopt(self)  # (closed with the context at the latest)

    def close(self) -> None:
        with self._lock:
            p, self._p = self._p, None
            if p is not None and p.value and self.ctx._h:
                self.array = None
                check(self.ctx._lib.pg_host_free(self.ctx._h, p))

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 — interpreter shutdown / a context that is gone already
            pass


class SeqSet(_Owner):
    """The contigs of one FASTA, 2-bit packed in HBM."""

    def __init__(self, ctx: Context, lens: Sequence[int]):
        self.ctx = ctx
        self._lib = ctx._lib
        self.lens = np.asarray(lens, dtype=np.uint64)
        self.names = [""] * len(self.lens)
        h = C.c_void_p()
        check(self._lib.pg_seqset_create(ctx._h, len(self.lens), _ptr(self.lens), C.byref(h)))
        self._h = h
        ctx._adopt(self)

    @classmethod
    def from_host(cls, ctx: Context, seqs: Sequence) -> "SeqSet":
        views = [_bytes_view(s) for s in seqs]
        ss = cls(ctx, [len(v) for v in views])
        for i, v in enumerate(views):
            ss.load_host(i, v)
        return ss

    @classmethod
    def from_fasta(cls, ctx: Context, source) -> "SeqSet":
        """FASTA file (path; ``.gz``/``.bgz`` through gzip) or FASTA text (bytes / uint8 array):
        the GPU strips the line breaks and packs; ``names`` / ``lens`` describe the records."""
        if isinstance(source, (str, os.PathLike)):
            path = os.fspath(source)
            if path.endswith((".gz", ".bgz")):
                import gzip
                with gzip.open(path, "rb") as f:
                    text = np.frombuffer(f.read(), dtype=np.uint8)
            else:
                text = np.fromfile(path, dtype=np.uint8)
        else:
            text = _bytes_view(source)
        ss = cls.__new__(cls)
        ss.ctx, ss._lib = ctx, ctx._lib
        h = C.c_void_p()
        check(ss._lib.pg_seqset_from_fasta(ctx._h, _ptr(text), len(text), C.byref(h)))
        ss._h = h
        ctx._adopt(ss)
        n = int(ss._lib.pg_seqset_ncontigs(h))
        lens, need = np.zeros(n, np.uint64), C.c_uint64()
        check(ss._lib.pg_seqset_describe(h, _ptr(lens), None, 0, C.byref(need)))  # (all contigs in two calls, not one each)
        buf = np.zeros(max(1, need.value), np.uint8)
        check(ss._lib.pg_seqset_describe(h, None, _ptr(buf), buf.size, None))
        names = buf[:need.value].tobytes().decode("latin-1").split("\0")[:n] if n else []
        ss.names, ss.lens = names, lens
        return ss

    @classmethod
    def from_fastq(cls, ctx: Context, source) -> Tuple["SeqSet", int, int]:
        """``(seqset, nreads, consumed)`` of FASTQ text (bytes / uint8 array) that starts at the first byte of a record, four
        lines per record (multi-line FASTQ is not supported): ONE contig, the sequence lines of all complete records joined by a
        single ``N`` on the GPU (pg_fastq.hip), ``names == [""]``; ``consumed`` = the offset just past the last complete record —
        the rest is a torn record for the next batch.  Without a complete record the contig has length 0.  A complete record
        whose line 0 does not begin with ``@`` or whose line 2 does not begin with ``+`` raises with code -1."""
        text = _bytes_view(source)
        ss = cls.__new__(cls)
        ss.ctx, ss._lib = ctx, ctx._lib
        h, nreads, consumed = C.c_void_p(), C.c_uint64(), C.c_uint64()
        check(ss._lib.pg_seqset_from_fastq(ctx._h, _ptr(text) if len(text) else None, len(text), C.byref(h), C.byref(nreads),
                                           C.byref(consumed)))
        ss._h = h
        ctx._adopt(ss)
        lens = np.zeros(1, np.uint64)
        check(ss._lib.pg_seqset_describe(h, _ptr(lens), None, 0, None))
        ss.names, ss.lens = [""], lens
        return ss, int(nreads.value), int(consumed.value)

    @classmethod
    def concat(cls, ctx: Context, sets: Sequence["SeqSet"]) -> "SeqSet":
        """One seqset with the contigs of all ``sets`` in order (device copy), for a co-scheduled
        result over several anchor genomes."""
        ss = cls.__new__(cls)
        ss.ctx, ss._lib = ctx, ctx._lib
        arr = (C.c_void_p * len(sets))(*[x._h for x in sets])
        h = C.c_void_p()
        check(ss._lib.pg_seqset_concat(ctx._h, arr, len(sets), C.byref(h)))
        ss._h = h
        ctx._adopt(ss)
        ss.names = [n for x in sets for n in x.names]
        ss.lens = np.concatenate([x.lens for x in sets]) if sets else np.zeros(0, np.uint64)
        return ss

    @classmethod
    def concat_ranges(cls, ctx: Context, parts: Sequence[Tuple["SeqSet", int, int]]) -> "SeqSet":
        """One seqset from contig ranges ``(set, first contig, count)``, in order (a set may appear several times)."""
        ss = cls.__new__(cls)
        ss.ctx, ss._lib = ctx, ctx._lib
        n = len(parts)
        arr = (C.c_void_p * n)(*[p[0]._h for p in parts])
        first = np.array([p[1] for p in parts], np.uint32)
        cnt = np.array([p[2] for p in parts], np.uint32)
        h = C.c_void_p()
        check(ss._lib.pg_seqset_concat_ranges(ctx._h, arr, _ptr(first), _ptr(cnt), n, C.byref(h)))
        ss._h = h
        ctx._adopt(ss)
        ss.names = [nm for s_, f, c in parts for nm in s_.names[f:f + c]]
        ss.lens = (np.concatenate([np.asarray(s_.lens[f:f + c], np.uint64) for s_, f, c in parts])
                   if parts else np.zeros(0, np.uint64))
        return ss

    def slice(self, pieces: Sequence[Tuple[int, int, int]]) -> "SeqSet":
        """A seqset of pieces ``(contig, start base, bases)`` of this one's contigs (starts: multiples of 32), packed
        planes copied on the device: the contig-sharded multi-GPU mode's chunks of long chromosomes.  A piece that
        carries ``k - 1`` bases of overlap holds exactly the k-mer positions ``[start, start + bases - k + 1)`` of its
        contig (cpp/anchor.cpp:127 cuts its chunks the same way)."""
        ss = SeqSet.__new__(SeqSet)
        ss.ctx, ss._lib = self.ctx, self._lib
        n = len(pieces)
        contig = np.array([p[0] for p in pieces], np.uint32)
        start = np.array([p[1] for p in pieces], np.uint64)
        lens = np.array([p[2] for p in pieces], np.uint64)
        h = C.c_void_p()
        check(self._lib.pg_seqset_slice(self.ctx._h, self._h, n, _ptr(contig), _ptr(start), _ptr(lens), C.byref(h)))
        ss._h = h
        self.ctx._adopt(ss)
        ss.names = [f"{self.names[c]}:{s0}" for c, s0, _ in pieces]
        ss.lens = lens
        return ss

    def load_host(self, idx: int, seq) -> None:
        v = _bytes_view(seq)
        check(self._lib.pg_seqset_load_host(self._h, idx, _ptr(v), len(v)))

    def unpack(self, idx: int) -> bytes:
        """contig idx as the kernels see it: ACGT upper case, N for every non-ACGT byte"""
        out = np.empty(int(self.lens[idx]), np.uint8)
        check(self._lib.pg_seqset_unpack(self._h, idx, _ptr(out)))
        return out.tobytes()

    def load_dev(self, idx: int, dev_ptr: int, length: int) -> None:
        check(self._lib.pg_seqset_load_dev(self._h, idx, C.c_void_p(dev_ptr), length))

    def total_kmers(self, k: int) -> int:
        return int(self._lib.pg_seqset_total_kmers(self._h, k))

    def close(self) -> None:
        if self._h:
            self._close_children()
            self._lib.pg_seqset_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KmerSketch:
    """Distinct canonical k-mers of a set of inputs before any table exists (HyperLogLog on the GPU,
    standard error 0.4 %): ``PanTable(..., expected_keys=sketch.estimate())`` is then sized once."""

    def __init__(self, ctx: Context, k: int):
        self.ctx, self._lib, self.k = ctx, ctx._lib, k
        h = C.c_void_p()
        check(self._lib.pg_sketch_create(ctx._h, k, C.byref(h)))
        self._h = h
        ctx._adopt(self)

    def add(self, seqs: SeqSet) -> None:
        check(self._lib.pg_sketch_add_seqset(self._h, seqs._h))

    def estimate(self) -> int:
        n = C.c_uint64()
        check(self._lib.pg_sketch_estimate(self._h, C.byref(n)))
        return int(n.value)

    def registers(self) -> np.ndarray:
        out = np.empty(65536, np.uint8)
        check(self._lib.pg_sketch_registers(self._h, _ptr(out)))
        return out

    def reset(self) -> None:
        check(self._lib.pg_sketch_reset(self._h))

    @staticmethod
    def estimate_registers(regs: np.ndarray) -> int:
        """estimate for register values held on the host — e.g. the register-wise maximum of several sketches
        (= the sketch of the union of their inputs)"""
        regs = np.ascontiguousarray(regs, np.uint8)
        if regs.size != 65536:
            raise ValueError("a sketch has 65536 registers")
        n = C.c_uint64()
        check(_lib.load().pg_sketch_estimate_registers(_ptr(regs), C.byref(n)))
        return int(n.value)

    def close(self) -> None:
        if self._h:
            self._lib.pg_sketch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MinHashSketch:
    """Bottom-s MinHash sketch of a sample on the GPU — the s smallest distinct h1 of MurmurHash3_x64_128 (seed 42) over
    the canonical 21-mers, what `mash sketch -s 10000` keeps (the reference workflow's genome_dist.tsv,
    panagram/workflow/Snakefile:124-149).  ``distinct``: the sample's distinct k-mer estimate (KmerSketch), which sets the
    candidate threshold; ``tau`` / ``capacity`` (0: automatic) force the threshold and the candidate buffer (tests of
    the reruns).  Several ``add`` calls make one sketch of their union."""

    K, S, SEED = 21, 10000, 42

    def __init__(self, ctx: Context, k: int = K, s: int = S, seed: int = SEED, tau: int = 0, capacity: int = 0):
        self.ctx, self._lib, self.k, self.s = ctx, ctx._lib, k, s
        h = C.c_void_p()
        check(self._lib.pg_minhash_create(ctx._h, k, s, seed, tau, capacity, C.byref(h)))
        self._h = h
        ctx._adopt(self)

    def add(self, seqs: SeqSet, distinct: int = 0) -> None:
        check(self._lib.pg_minhash_add_seqset(self._h, seqs._h, int(distinct)))

    def result(self) -> Tuple[np.ndarray, int]:
        """(the sketch: ascending uint64, at most s values; ACGT bases added)"""
        out = np.empty(self.s, np.uint64)
        n, bases = C.c_uint32(), C.c_uint64()
        check(self._lib.pg_minhash_result(self._h, _ptr(out), C.byref(n), C.byref(bases), None))
        return out[:n.value].copy(), int(bases.value)

    def passes(self) -> int:
        """kernel launches since creation / reset (1 per sample unless a rerun was needed)"""
        n, p = C.c_uint32(), C.c_uint32()
        check(self._lib.pg_minhash_result(self._h, None, C.byref(n), None, C.byref(p)))
        return int(p.value)

    def reset(self) -> None:
        check(self._lib.pg_minhash_reset(self._h))

    def close(self) -> None:
        if self._h:
            self._lib.pg_minhash_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def minhash_distances(sketches: Sequence[np.ndarray], bases: Optional[Sequence[int]] = None, s: int = MinHashSketch.S,
                      k: int = MinHashSketch.K):
    """Every pair i < j of sketches, in the order (0,1) (0,2) .. (1,2) ..: (distance, p-value, common, denom) arrays —
    mash's compareSketches (host only, no device).  ``bases``: ACGT bases per sample for the p-values (None: all 1)."""
    n = len(sketches)
    offsets = np.zeros(n + 1, np.uint64)
    offsets[1:] = np.cumsum([len(x) for x in sketches])
    hashes = np.ascontiguousarray(np.concatenate([np.asarray(x, np.uint64) for x in sketches]) if n else np.zeros(0, np.uint64))
    npairs = n * (n - 1) // 2
    dist, pval = np.empty(npairs, np.float64), np.empty(npairs, np.float64)
    common, denom = np.empty(npairs, np.uint32), np.empty(npairs, np.uint32)
    b = None if bases is None else np.ascontiguousarray(bases, np.uint64)
    if b is not None and b.size != n:
        raise ValueError("one base count per sketch")
    check(_lib.load().pg_minhash_distances(_ptr(hashes), _ptr(offsets), n, s, k, _ptr(b), _ptr(dist), _ptr(pval), _ptr(common),
                                           _ptr(denom)))
    return dist, pval, common, denom


def knn_rows(ctx: Context, X, k: int, seg=None) -> Tuple[np.ndarray, np.ndarray]:
    """(idx [n, k] int32, d2 [n, k] float32): the k nearest rows of every row of the n x D float32 matrix ``X`` under squared
    Euclidean distance, exact (k_knn_rows, one launch).  ``seg``: ascending row offsets from 0 to n — a row searches only the
    rows of its own segment, itself included (None: one segment).  Entries are sorted by (d2, row number); d2 is the float32
    sum over the columns in order, each subtract, multiply and add rounded; (-1, inf) pads a segment of fewer than k rows."""
    X = np.ascontiguousarray(X, np.float32)
    if X.ndim != 2:
        raise ValueError("X must be a matrix")
    n, D = X.shape
    s = None if seg is None else np.ascontiguousarray(seg, np.uint64)
    if s is not None and (s.ndim != 1 or len(s) < 1):
        raise ValueError("seg needs at least one offset")
    idx = np.empty((n, int(k) if 0 < int(k) <= 32 else 0), np.int32)
    d2 = np.empty(idx.shape, np.float32)
    check(ctx._lib.pg_knn_rows(ctx._h, _ptr(X), n, D, int(k), _ptr(s), 0 if s is None else len(s) - 1, _ptr(idx), _ptr(d2)))
    return idx, d2


NO_MATE = 0xFFFFFFFF


class PosTable:
    """Position table of two sequence sets in HBM (pg_synteny.hip): per distinct canonical k-mer the position of its one
    occurrence in side 0 (A) and in side 1 (B), or a mark that the side holds it more than once.  ``capacity_keys``: the distinct
    keys it must hold — the k-mer positions of both sides always suffice.  A side whose keys do not fit raises with code -4
    (PG_E_CAPACITY); the table is then of no further use.  For ``hit_runs`` and ``locate`` (pg_locate.hip) side 1 holds query
    sequences, side 0 stays empty, and any sequence set is streamed through the table: the queries' k-mer positions suffice."""

    def __init__(self, ctx: Context, k: int, capacity_keys: int):
        self.ctx, self._lib, self.k = ctx, ctx._lib, int(k)
        h = C.c_void_p()
        check(self._lib.pg_postable_create(ctx._h, int(k), int(capacity_keys), C.byref(h)))
        self._h = h
        ctx._adopt(self)

    def insert(self, side: int, seqs: SeqSet) -> None:
        check(self._lib.pg_postable_insert_seqset(self._h, int(side), seqs._h))

    def mates(self, seqs_a: SeqSet, download: bool = True):
        """(mate word of every k-mer position of ``seqs_a`` — the set inserted as side 0 — contigs back to back: ``posB << 1 |
        strand``, NO_MATE where the k-mer is not unique in both sides; the mated positions).  ``download=False``: None in
        place of the array, which then only stays in HBM."""
        out = np.empty(seqs_a.total_kmers(self.k), np.uint32) if download else None
        n = C.c_uint64()
        check(self._lib.pg_postable_mates(self._h, seqs_a._h, _ptr(out), C.byref(n)))
        return out, int(n.value)

    def hit_runs(self, seqs: SeqSet, cap: Optional[int] = None):
        """(run_contig, run_start, run_end, run_hit, runs per contig, hit positions per contig): the maximal collinear runs of the
        hits of ``seqs`` — any sequence set, streamed through the table — in side 1 (the queries).  A position has a hit when its
        k-mer occurs exactly once in side 1, however often ``seqs`` holds it: ``run_hit`` = ``posQ << 1 | strand`` of the run's
        first position, positions of ``seqs`` contig-relative; sorted by (contig, start).  The queries themselves as ``seqs``: hits
        per contig = every query's unique k-mers.  ``cap`` (tests of the capacity protocol): ONE call with arrays of ``cap``
        entries, returned whole behind the total and the hits."""
        n = len(seqs.lens)
        per, hits, total, nhits = np.zeros(n, np.uint64), np.zeros(n, np.uint64), C.c_uint64(), C.c_uint64()

        def call(m):
            arrs = [np.full(m, NO_MATE, np.uint32) for _ in range(4)]
            check(self._lib.pg_postable_hit_runs(self._h, seqs._h, m, *[_ptr(a) if m else None for a in arrs], _ptr(per) if n else None,
                                                 _ptr(hits) if n else None, C.byref(total), C.byref(nhits)))
            return arrs
        if cap is not None:
            arrs = call(int(cap))
            return (*arrs, per, hits, int(total.value), int(nhits.value))
        call(0)
        arrs = call(int(total.value))
        return (*arrs, per, hits)

    def locate(self, seqs_g: SeqSet, seqs_q: SeqSet, min_run: int = 1, max_gap: int = 1000, max_shift: int = 100,
               cap: Optional[int] = None):
        """(the eight block arrays of ``run_blocks``, blocks per contig of ``seqs_g``, hit positions, runs): the hit runs of
        ``seqs_g`` chained into blocks against ``seqs_q``, which must be the set inserted as side 1 — A is ``seqs_g``, B the
        queries; runs and hits never leave HBM.  ``cap``: the blocks expected (a second call follows when there are more)."""
        params = _block_params(min_run, max_gap, max_shift)
        ng = len(seqs_g.lens)
        per, total, nhits, nruns = np.zeros(ng, np.uint64), C.c_uint64(), C.c_uint64(), C.c_uint64()
        n = int(cap) if cap is not None else 4096
        while True:
            arrs = [np.empty(n, np.uint32) for _ in range(8)]
            check(self._lib.pg_postable_locate(self._h, seqs_g._h, seqs_q._h, *params, n, *[_ptr(a) if n else None for a in arrs],
                                               _ptr(per) if ng else None, C.byref(total), C.byref(nhits), C.byref(nruns)))
            if int(total.value) <= n:
                break
            n = int(total.value)
        return (*[a[:total.value].copy() for a in arrs], per, int(nhits.value), int(nruns.value))

    def close(self) -> None:
        if self._h:
            self._lib.pg_postable_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def mate_runs(ctx: Context, mates, nkmers, cap: Optional[int] = None):
    """(run_contig, run_start, run_end, run_mate, runs per contig): the maximal collinear runs of an array of mate words
    (``nkmers[c]`` entries per contig, back to back) — per run its contig, first position and exclusive end inside the contig,
    and the mate word of its first position; sorted by (contig, start).  ``cap`` (tests of the capacity protocol): ONE call with
    arrays of ``cap`` entries, returned whole behind the total."""
    m = np.ascontiguousarray(mates, np.uint32)
    nk = np.ascontiguousarray(nkmers, np.uint64)
    if m.ndim != 1 or nk.ndim != 1 or int(nk.sum()) != m.size:
        raise ValueError("one mate word per k-mer position of every contig")
    per, total = np.zeros(len(nk), np.uint64), C.c_uint64()

    def call(n):
        arrs = [np.full(n, NO_MATE, np.uint32) for _ in range(4)]
        check(ctx._lib.pg_mate_runs(ctx._h, _ptr(m), len(nk), _ptr(nk), n, *[_ptr(a) if n else None for a in arrs], _ptr(per),
                                    C.byref(total)))
        return arrs
    if cap is not None:
        arrs = call(int(cap))
        return (*arrs, per, int(total.value))
    call(0)
    arrs = call(int(total.value))
    return (*arrs, per)


def synteny_segments(ctx: Context, k: int, seqs_a: SeqSet, seqs_b: SeqSet, cap: Optional[int] = None):
    """(run_contig, run_start, run_end, run_mate, runs per contig of A, mated positions of A): the maximal collinear runs of
    k-mers that occur exactly once in ``seqs_a`` and exactly once in ``seqs_b``, as ``mate_runs`` returns them — table, mates
    and runs in one library call, the mates never leaving HBM.  ``cap``: the runs expected (a second call follows when there
    are more)."""
    per, total, nmated = np.zeros(len(seqs_a.lens), np.uint64), C.c_uint64(), C.c_uint64()
    n = int(cap) if cap is not None else max(1024, min(1 << 20, seqs_a.total_kmers(k) // 16))
    while True:
        arrs = [np.empty(n, np.uint32) for _ in range(4)]
        check(ctx._lib.pg_synteny_segments(ctx._h, int(k), seqs_a._h, seqs_b._h, n, *[_ptr(a) if n else None for a in arrs], _ptr(per),
                                           C.byref(total), C.byref(nmated)))
        if int(total.value) <= n:
            break
        n = int(total.value)
    return (*[a[:total.value].copy() for a in arrs], per, int(nmated.value))


def synteny_counts(ctx: Context, k: int, seqs_a: SeqSet, seqs_b: SeqSet) -> Tuple[int, int]:
    """(runs, mated positions of A) of ``synteny_segments`` without the runs: one call that emits nothing.  A set against itself
    counts the positions whose k-mer is unique in it."""
    per, total, nmated = np.zeros(len(seqs_a.lens), np.uint64), C.c_uint64(), C.c_uint64()
    check(ctx._lib.pg_synteny_segments(ctx._h, int(k), seqs_a._h, seqs_b._h, 0, None, None, None, None, _ptr(per), C.byref(total),
                                       C.byref(nmated)))
    return int(total.value), int(nmated.value)


def synteny_last_timing() -> dict:
    """HIP-event milliseconds of the kernels of this thread's last ``synteny_segments`` call"""
    ms = (C.c_float * 5)()
    check(_lib.load().pg_synteny_last_timing(ms))
    return dict(zip(("insert_a_ms", "insert_b_ms", "mates_ms", "runs_count_ms", "runs_emit_ms"), (float(x) for x in ms)))


BLOCK_FIELDS = ("contig", "start", "end", "mate_first", "mate_last", "kmers", "runs", "shifted")


def _block_params(min_run, max_gap, max_shift):
    vals = [int(min_run), int(max_gap), int(max_shift)]
    if any(not 0 <= v < 1 << 32 for v in vals):  # (the library's own limits are narrower: it answers PG_E_INVALID for those)
        raise ValueError("min_run, max_gap and max_shift are 32-bit counts")
    return vals


def run_blocks(ctx: Context, run_contig, run_start, run_end, run_mate, ncontigs_a: int, lens_b, min_run: int = 1, max_gap: int = 1000,
               max_shift: int = 100, cap: Optional[int] = None):
    """(contig, start, end, mate_first, mate_last, kmers, runs, shifted, blocks per contig of A): the runs of ``mate_runs`` /
    ``synteny_segments`` chained on the GPU into blocks — maximal chains of runs of at least ``min_run`` k-mers on one strand,
    each at most ``max_gap`` positions behind its predecessor on both genomes with the two distances at most ``max_shift`` apart,
    inside one contig of B (``lens_b``: the lengths of B's contigs); the definitions are include/panagram_hip.h's.  Sorted by
    (contig, start).  ``cap`` (tests of the capacity protocol): ONE call with arrays of ``cap`` entries, returned whole behind
    the total."""
    rc, rs, re_, rm = (np.ascontiguousarray(x, np.uint32) for x in (run_contig, run_start, run_end, run_mate))
    if not (rc.ndim == 1 and rc.shape == rs.shape == re_.shape == rm.shape):
        raise ValueError("the run arrays differ in length")
    lb = np.ascontiguousarray(lens_b, np.uint64)
    params = _block_params(min_run, max_gap, max_shift)
    per, total = np.zeros(int(ncontigs_a), np.uint64), C.c_uint64()

    def call(n):
        arrs = [np.full(n, NO_MATE, np.uint32) for _ in range(8)]
        check(ctx._lib.pg_run_blocks(ctx._h, _ptr(rc), _ptr(rs), _ptr(re_), _ptr(rm), len(rc), len(per), len(lb), _ptr(lb), *params, n,
                                     *[_ptr(a) if n else None for a in arrs], _ptr(per), C.byref(total)))
        return arrs
    if cap is not None:
        arrs = call(int(cap))
        return (*arrs, per, int(total.value))
    call(0)
    arrs = call(int(total.value))
    return (*arrs, per)


def synteny_blocks(ctx: Context, k: int, seqs_a: SeqSet, seqs_b: SeqSet, min_run: int = 1, max_gap: int = 1000, max_shift: int = 100,
                   cap: Optional[int] = None):
    """(the eight block arrays of ``run_blocks``, blocks per contig of A, mated positions of A, runs): the blocks of the unique
    matches of ``seqs_a`` in ``seqs_b`` — table, mates, runs and blocks in one library call; the mates and the runs never leave
    HBM.  ``cap``: the blocks expected (a second call follows when there are more)."""
    params = _block_params(min_run, max_gap, max_shift)
    per, total, nmated, nruns = np.zeros(len(seqs_a.lens), np.uint64), C.c_uint64(), C.c_uint64(), C.c_uint64()
    n = int(cap) if cap is not None else 4096
    while True:
        arrs = [np.empty(n, np.uint32) for _ in range(8)]
        check(ctx._lib.pg_synteny_blocks(ctx._h, int(k), seqs_a._h, seqs_b._h, *params, n, *[_ptr(a) if n else None for a in arrs],
                                         _ptr(per), C.byref(total), C.byref(nmated), C.byref(nruns)))
        if int(total.value) <= n:
            break
        n = int(total.value)
    return (*[a[:total.value].copy() for a in arrs], per, int(nmated.value), int(nruns.value))


def synteny_blocks_last_timing() -> dict:
    """HIP-event milliseconds of the kernels of this thread's last ``synteny_blocks`` call"""
    ms = (C.c_float * 7)()
    check(_lib.load().pg_synteny_blocks_last_timing(ms))
    return dict(zip(("insert_a_ms", "insert_b_ms", "mates_ms", "runs_count_ms", "runs_emit_ms", "blocks_count_ms", "blocks_emit_ms"),
                    (float(x) for x in ms)))


VARIANT_FIELDS = ("contig", "posA", "lenA", "posB", "lenB", "info", "mismatches", "alleleA", "alleleB")
VARIANT_CLASSES = ("same", "snp", "mnp", "ins", "del", "complex")


def _variant_arrays(n):
    return [np.full(n, NO_MATE, np.uint32) for _ in range(7)] + [np.full(n, (1 << 64) - 1, np.uint64) for _ in range(2)]


def run_variants(ctx: Context, k: int, seqs_a: SeqSet, seqs_b: SeqSet, run_contig, run_start, run_end, run_mate, min_run: int = 1,
                 max_gap: int = 1000, max_shift: int = 100, cap: Optional[int] = None):
    """(contig, posA, lenA, posB, lenB, info, mismatches, alleleA, alleleB, class counts [6], links): the links of the blocks that
    ``run_blocks`` chains from these runs as variants of ``seqs_b`` against ``seqs_a`` — every link classified (``VARIANT_CLASSES``),
    compared base by base on the GPU and, unless its class is ``same``, emitted with its place on both genomes and the first 32
    bases of both alleles in A's orientation; the definitions are include/panagram_hip.h's.  ``info`` = strand | class << 1 | code
    of the anchor base << 4 | N flag << 6.  Sorted by (contig, posA).  ``links`` counts all links, class 0 included.  ``cap``
    (tests of the capacity protocol): ONE call with arrays of ``cap`` entries, returned whole behind the total."""
    rc, rs, re_, rm = (np.ascontiguousarray(x, np.uint32) for x in (run_contig, run_start, run_end, run_mate))
    if not (rc.ndim == 1 and rc.shape == rs.shape == re_.shape == rm.shape):
        raise ValueError("the run arrays differ in length")
    params = _block_params(min_run, max_gap, max_shift)
    cls, links, total = np.zeros(6, np.uint64), C.c_uint64(), C.c_uint64()

    def call(n):
        arrs = _variant_arrays(n)
        check(ctx._lib.pg_run_variants(ctx._h, int(k), seqs_a._h, seqs_b._h, _ptr(rc), _ptr(rs), _ptr(re_), _ptr(rm), len(rc), *params, n,
                                       *[_ptr(a) if n else None for a in arrs], _ptr(cls), C.byref(links), C.byref(total)))
        return arrs
    if cap is not None:
        arrs = call(int(cap))
        return (*arrs, cls, int(links.value), int(total.value))
    call(0)
    arrs = call(int(total.value))
    return (*arrs, cls, int(links.value))


def synteny_variants(ctx: Context, k: int, seqs_a: SeqSet, seqs_b: SeqSet, min_run: int = 1, max_gap: int = 1000, max_shift: int = 100,
                     cap: Optional[int] = None):
    """(the nine record arrays of ``run_variants``, class counts [6], links, mated positions of A, runs, blocks): the variants of
    ``seqs_b`` against ``seqs_a`` inside the blocks of their unique matches — table, mates, runs, blocks and variants in one
    library call; mates, runs and blocks never leave HBM.  ``cap``: the records expected (a second call follows when there are
    more)."""
    params = _block_params(min_run, max_gap, max_shift)
    cls, links, total = np.zeros(6, np.uint64), C.c_uint64(), C.c_uint64()
    nmated, nruns, nblocks = C.c_uint64(), C.c_uint64(), C.c_uint64()
    n = int(cap) if cap is not None else 4096
    while True:
        arrs = _variant_arrays(n)
        check(ctx._lib.pg_synteny_variants(ctx._h, int(k), seqs_a._h, seqs_b._h, *params, n, *[_ptr(a) if n else None for a in arrs],
                                           _ptr(cls), C.byref(links), C.byref(total), C.byref(nmated), C.byref(nruns), C.byref(nblocks)))
        if int(total.value) <= n:
            break
        n = int(total.value)
    return (*[a[:total.value].copy() for a in arrs], cls, int(links.value), int(nmated.value), int(nruns.value), int(nblocks.value))


def synteny_variants_last_timing() -> dict:
    """HIP-event milliseconds of the kernels of this thread's last ``synteny_variants`` call"""
    ms = (C.c_float * 9)()
    check(_lib.load().pg_synteny_variants_last_timing(ms))
    return dict(zip(("insert_a_ms", "insert_b_ms", "mates_ms", "runs_count_ms", "runs_emit_ms", "blocks_count_ms", "blocks_emit_ms",
                     "variants_count_ms", "variants_emit_ms"), (float(x) for x in ms)))


def locate_last_timing() -> dict:
    """HIP-event milliseconds of the kernels of this thread's last ``PosTable.locate`` (``hit_runs``: the first two)"""
    ms = (C.c_float * 4)()
    check(_lib.load().pg_locate_last_timing(ms))
    return dict(zip(("hits_count_ms", "hits_emit_ms", "blocks_count_ms", "blocks_emit_ms"), (float(x) for x in ms)))


COPIES_BINS = 64  # depth bins of a copy-number histogram: bin c = depth c, the last = that depth and beyond
COPIES_CHUNK = 4096
PLACE_CHUNK = 4096   # rows a workgroup of k_sample_agree takes
FASTQ_TILE = 4096    # bytes of text a workgroup of k_fastq_scan / k_fastq_join takes
DEPTH_INVALID = 0xFFFF  # a position of a depth track whose window holds a non-ACGT base


class CopyTable:
    """Count table of target k-mers in HBM (pg_copies.hip): the distinct canonical k-mers of the inserted sequence sets, and
    ``nplanes`` planes of one 32-bit counter per key — one plane per genome counted.  ``capacity_keys``: the distinct keys it must
    hold — the targets' k-mer positions always suffice.  Targets whose keys do not fit raise with code -4 (PG_E_CAPACITY); the
    table is then of no further use."""

    def __init__(self, ctx: Context, k: int, capacity_keys: int, nplanes: int = 1):
        self.ctx, self._lib, self.k, self.nplanes = ctx, ctx._lib, int(k), int(nplanes)
        h = C.c_void_p()
        check(self._lib.pg_copytable_create(ctx._h, int(k), int(capacity_keys), int(nplanes), C.byref(h)))
        self._h = h
        ctx._adopt(self)

    def insert(self, targets: SeqSet) -> int:
        """the keys of ``targets``' valid k-mers into the table (keys accumulate over calls); the keys this call added"""
        n = C.c_uint64()
        check(self._lib.pg_copytable_insert_seqset(self._h, targets._h, C.byref(n)))
        return int(n.value)

    def count(self, plane: int, genome: SeqSet) -> int:
        """every valid k-mer of ``genome`` whose key the table holds adds 1 to that key's counter in ``plane``; how many did"""
        if plane < 0:
            raise ValueError(f"plane {plane}")
        n = C.c_uint64()
        check(self._lib.pg_copytable_count_seqset(self._h, int(plane), genome._h, C.byref(n)))
        return int(n.value)

    def clear(self, plane: int) -> None:
        if plane < 0:
            raise ValueError(f"plane {plane}")
        check(self._lib.pg_copytable_clear_plane(self._h, int(plane)))

    def profile(self, seqs: SeqSet, plane0: int = 0, nplanes: Optional[int] = None, track: bool = False):
        """(hist [contigs, planes, COPIES_BINS] uint64, valid [contigs] uint64[, depths [planes, k-mer positions] uint16]) of the
        contigs of ``seqs`` — any sequence set, a key the table does not hold reads depth 0 — in planes ``plane0 .. plane0 +
        nplanes - 1`` (None: all from plane0 on).  hist[t, g, c] = the valid positions of contig t whose k-mer genome g holds
        min(depth, 63) == c times; depths: min(depth, 65534) per position, the contigs back to back, DEPTH_INVALID where the
        window holds a non-ACGT base."""
        npl = self.nplanes - int(plane0) if nplanes is None else int(nplanes)
        if plane0 < 0 or npl < 0:
            raise ValueError(f"planes {plane0}, {nplanes}")
        n = len(seqs.lens)
        hist, valid = np.zeros((n, max(npl, 0), COPIES_BINS), np.uint64), np.zeros(n, np.uint64)
        total = seqs.total_kmers(self.k)
        depths = np.zeros((max(npl, 0), total), np.uint16) if track else None
        pad = np.zeros(1, np.uint64)  # (a set without a contig: the library still wants somewhere to point)
        check(self._lib.pg_copytable_profile(self._h, seqs._h, int(plane0), npl, _ptr(hist if hist.size else pad),
                                             _ptr(valid if n else pad), _ptr(depths if depths is None or depths.size else pad)))
        return (hist, valid, depths) if track else (hist, valid)

    def sample_agree(self, plane: int, min_count: int, anchor: SeqSet, rows: "AnchorResult", contigs, starts, ends):
        """(valid [windows], held [windows], col [windows, genomes], both [windows, genomes]) uint64 of windows ``[starts[i],
        ends[i])`` of the rows of contig ``contigs[i]`` of ``rows``, whose row r is the k-mer at bases ``[r, r + k)`` of that
        contig of ``anchor``: the valid rows, those whose k-mer ``plane`` counted at least ``min_count`` times (the sample holds
        it), those with genome g's bit, and those with both (pg_place.hip: one launch family, nothing per position comes back)."""
        if plane < 0 or min_count < 0:
            raise ValueError(f"plane {plane}, min_count {min_count}")
        contigs, starts, ends = _windows(contigs, starts, ends, "window")
        n, N = len(contigs), rows.ngenomes
        valid, held = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        col, both = np.zeros((n, N), np.uint64), np.zeros((n, N), np.uint64)
        check(self._lib.pg_copytable_sample_agree(self._h, int(plane), int(min_count), anchor._h, rows._h, n, _ptr(contigs), _ptr(starts),
                                                  _ptr(ends), _ptr(valid), _ptr(held), _ptr(col), _ptr(both)))
        return valid, held, col, both

    def insert_ranges(self, seqs: SeqSet, contigs, starts, lens) -> int:
        """the keys of the allele windows of ranges ``(contigs[i], starts[i], lens[i])`` of ``seqs`` into the table — every k-mer
        window that overlaps bases ``[start, start + len)`` of that contig; ``len == 0`` is the junction in front of base
        ``start``, whose windows hold both its neighbours (pg_genotype.hip) — as ``insert`` puts whole contigs in, without a
        contig cut per range; the keys this call added"""
        contigs, starts, lens = _windows(contigs, starts, lens, "range")
        n = C.c_uint64()
        check(self._lib.pg_copytable_insert_ranges(self._h, seqs._h, len(contigs), _ptr(contigs), _ptr(starts), _ptr(lens), C.byref(n)))
        return int(n.value)

    def allele_support(self, seqs: SeqSet, contigs, starts, lens, own: int, other: int, sample: int, min_count: int):
        """(windows, inf, seen, depth) uint64 per range ``(contigs[i], starts[i], lens[i])`` of ``seqs``: its allele windows that
        exist; the informative ones, whose k-mer plane ``own`` counted exactly once and plane ``other`` never; those of them plane
        ``sample`` counted at least ``min_count`` times; and the sum of ``sample``'s counts over the informative ones (one launch
        family, four integers per range come back: pg_genotype.hip).  A k-mer the table does not hold is never informative."""
        if min(own, other, sample) < 0 or min_count < 0:
            raise ValueError(f"planes {own}, {other}, {sample}, min_count {min_count}")
        contigs, starts, lens = _windows(contigs, starts, lens, "range")
        n = len(contigs)
        out = [np.zeros(n, np.uint64) for _ in range(4)]
        check(self._lib.pg_copytable_allele_support(self._h, seqs._h, n, _ptr(contigs), _ptr(starts), _ptr(lens), int(own), int(other),
                                                    int(sample), int(min_count), *[_ptr(x) for x in out]))
        return tuple(out)

    @staticmethod
    def genotype_last_timing() -> dict:
        return genotype_last_timing()

    def close(self) -> None:
        if self._h:
            self._lib.pg_copytable_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def copies_last_timing() -> dict:
    """HIP-event milliseconds of k_copy_insert, k_copy_count and k_copy_profile in this thread's last ``CopyTable`` calls"""
    ms = (C.c_float * 3)()
    check(_lib.load().pg_copies_last_timing(ms))
    return dict(zip(("insert_ms", "count_ms", "profile_ms"), (float(x) for x in ms)))


def genotype_last_timing() -> dict:
    """HIP-event milliseconds of k_allele_insert and k_allele_support in this thread's last ``CopyTable.insert_ranges`` and
    ``CopyTable.allele_support``"""
    ms = (C.c_float * 2)()
    check(_lib.load().pg_genotype_last_timing(ms))
    return dict(zip(("insert_ms", "support_ms"), (float(x) for x in ms)))


def place_last_timing() -> dict:
    """HIP-event milliseconds of the kernels of this thread's last ``SeqSet.from_fastq`` (scan, offsets, join and pack together)
    and of k_sample_agree in its last ``CopyTable.sample_agree``"""
    ms = (C.c_float * 2)()
    check(_lib.load().pg_place_last_timing(ms))
    return dict(zip(("fastq_ms", "agree_ms"), (float(x) for x in ms)))


class PanTable(_Owner):
    """GPU-resident k-mer -> genome-mask table (replaces kmc/bitvec{i})."""

    def __init__(self, ctx: Context, k: int, ngenomes: int, expected_keys: int = 0, coscheduled: int = 0, keys_per_line: float = 0.0):
        """``coscheduled``: how many anchor genomes one probe launch will anchor side by side against this table (0: not
        known = several; 1: one genome per launch, no co-scheduling partner) — it decides the minimizer window with the
        key count (pg_table_set_coscheduled, include/panagram_hip.h).  ``keys_per_line`` (0: the library's 3): a denser
        table for a known ``expected_keys`` — pg_table_create_dense: the genome-sharded mode's block tables"""
        self.ctx = ctx
        self._lib = ctx._lib
        self.k, self.ngenomes = k, ngenomes
        self.nbytes = (ngenomes + 7) // 8
        self.ndbs = (ngenomes + 31) // 32
        h = C.c_void_p()
        if keys_per_line:
            check(self._lib.pg_table_create_dense(ctx._h, k, ngenomes, expected_keys, float(keys_per_line), C.byref(h)))
        else:
            check(self._lib.pg_table_create(ctx._h, k, ngenomes, expected_keys, C.byref(h)))
        self._h = h
        ctx._adopt(self)
        if coscheduled:
            self.set_coscheduled(coscheduled)

    # Densities a table may be created at when HBM is plentiful (round 6): the library's own 3 keys per 128-byte line date from
    # 80-GB parts; at 1.5 keys per line fewer keys sit outside their home line (8 x 100 Mb: 15.5 % -> 9.5 %), the overflow drain
    # of a tile is shorter and k_probe gains 3 % at 8 genomes, 5-6 % at 27-64 (profiles/r6k2_density_sweep.txt) for twice the table
    # bytes — 21 GB instead of 10 of an MI355X's 288.
    # Not for repeat-rich genomes: half of every genome in transposable-element families (bench.py's plant-like leg) runs 5 %
    # SLOWER against the sparser table (profiles/r6m_roomy_robustness.txt) — the lines of a repeat family are the ones that are
    # used again and again, and at half the density they are twice as many for the caches to hold.  ``distinct_fraction`` =
    # distinct k-mers / k-mer positions of ONE genome (its sketch) tells the two apart.
    ROOMY_DENSITIES = (1.25, 1.5, 2.0, 2.5)  # (1.25 against 1.5 at configs[1]: 3.154 against 3.206 ms, 1.0 no better: profiles/r6s_density_piece.txt)
    ROOMY_SHARE = 0.6       # of what is free beside ``other_bytes`` and the reserve
    ROOMY_RESERVE = 8 << 30
    ROOMY_MIN_DISTINCT = 0.85

    @classmethod
    def roomy_density(cls, ctx: Context, k: int, ngenomes: int, expected_keys: int, other_bytes: int = 0,
                      distinct_fraction: Optional[float] = None) -> float:
        """keys per line (0: the library's default) for a table of ``expected_keys`` that has ``other_bytes`` of HBM to leave
        alone (the rows it will be anchored into, buffers still to come): the sparsest of ROOMY_DENSITIES that fits into
        ROOMY_SHARE of the rest (more than 64 genomes, inline / split lines: the same load, 65 / 96 x 10 Mb -4 % / -20 % probe time,
        profiles/r6q_wide_density.txt); tables of unknown size and of repeat-rich genomes (``distinct_fraction`` of one genome
        below ROOMY_MIN_DISTINCT) keep the default"""
        if not expected_keys or os.environ.get("PG_TABLE_ROOMY", "1") in ("0", "") or os.environ.get("PG_TABLE_KEYS_PER_LINE"):
            return 0.0
        if distinct_fraction is not None and distinct_fraction < cls.ROOMY_MIN_DISTINCT:
            return 0.0
        room = (ctx.mem_info()[0] - int(other_bytes) - cls.ROOMY_RESERVE) * cls.ROOMY_SHARE
        for kpl in cls.ROOMY_DENSITIES:
            if cls.bytes_for(k, ngenomes, expected_keys, kpl) <= room:
                return kpl
        return 0.0

    def set_coscheduled(self, anchors: int) -> None:
        """tell an EMPTY table how it will be probed (see __init__)"""
        check(self._lib.pg_table_set_coscheduled(self._h, int(anchors)))

    @staticmethod
    def bytes_for(k: int, ngenomes: int, expected_keys: int, keys_per_line: float = 0.0) -> int:
        """device bytes a table created for that many keys (at that density; 0: the library's) takes"""
        b = C.c_uint64()
        if keys_per_line:
            check(_lib.load().pg_table_bytes_for_dense(k, ngenomes, expected_keys, float(keys_per_line), C.byref(b)))
        else:
            check(_lib.load().pg_table_bytes_for(k, ngenomes, expected_keys, C.byref(b)))
        return int(b.value)

    def insert_seqset(self, genome_idx: int, seqs: SeqSet, min_count: int = 1) -> None:
        """OR genome ``genome_idx``'s bit into every canonical k-mer of ``seqs`` that occurs at least
        ``min_count`` times in it (kmc -ci<min_count>; 2 for read sets)"""
        if min_count > 1:
            check(self._lib.pg_table_insert_seqset_min(self._h, genome_idx, seqs._h, min_count))
            return
        check(self._lib.pg_table_insert_seqset(self._h, genome_idx, seqs._h))

    def update_seqset(self, genome_idx: int, seqs: SeqSet) -> None:
        """OR genome ``genome_idx``'s bit into the k-mers of ``seqs`` that the table ALREADY holds; no key is added
        (a table of the anchors' k-mers only answers the anchor step like the table of all genomes)"""
        check(self._lib.pg_table_update_seqset(self._h, genome_idx, seqs._h))

    def clear(self) -> None:
        """empty the table, keeping its allocation (the next genome block is built in the same memory)"""
        check(self._lib.pg_table_clear(self._h))

    def insert_keys(self, db_idx: int, keys: np.ndarray, counters: np.ndarray) -> None:
        keys = np.ascontiguousarray(keys, np.uint64)
        counters = np.ascontiguousarray(counters, np.uint32)
        if len(keys) != len(counters):
            raise ValueError("keys and counters differ in length")
        check(self._lib.pg_table_insert_keys(self._h, db_idx, _ptr(keys), _ptr(counters), len(keys)))

    def load_kmc1(self, db_idx: int, pre: bytes, suf: bytes) -> None:
        """images of X.kmc_pre / X.kmc_suf (KMC1 or KMC2 layout) as 32-genome group ``db_idx``"""
        check(self._lib.pg_table_load_kmc(self._h, db_idx, pre, len(pre), suf, len(suf)))

    load_kmc = load_kmc1

    def load_kmc_files(self, db_idx: int, prefix: str) -> None:
        """``prefix.kmc_pre`` / ``prefix.kmc_suf`` as 32-genome group ``db_idx`` (CKMCFile::OpenForRA,
        cpp/anchor.cpp:29): the files are mapped, not read into Python"""
        pre = np.memmap(prefix + ".kmc_pre", dtype=np.uint8, mode="r")
        suf = np.memmap(prefix + ".kmc_suf", dtype=np.uint8, mode="r")
        check(self._lib.pg_table_load_kmc(self._h, db_idx, _ptr(pre), pre.size, _ptr(suf), suf.size))

    def stats(self) -> dict:
        v = [C.c_uint64() for _ in range(4)]
        check(self._lib.pg_table_stats(self._h, *[C.byref(x) for x in v]))
        return dict(nkeys=v[0].value, nslots=v[1].value, nbuckets=v[2].value, bytes=v[3].value)

    def kmer_stats(self) -> dict:
        """shared distinct k-mer counts of the k-mers the table was built from, one pass over its slots on the GPU
        (pg_table_pair_counts): ``pairs`` (N x N int64, symmetric: k-mers held by both genomes, the diagonal a genome's
        distinct k-mers), ``occupancy`` (N + 1: k-mers held by exactly n genomes), ``private`` (N: k-mers of one genome
        alone) and ``nkeys``"""
        n = self.ngenomes
        pairs = np.zeros((n, n), np.uint64)
        occ, priv, nkeys = np.zeros(n + 1, np.uint64), np.zeros(n, np.uint64), C.c_uint64()
        check(self._lib.pg_table_pair_counts(self._h, _ptr(pairs), _ptr(occ), _ptr(priv), C.byref(nkeys)))
        return dict(pairs=pairs.astype(np.int64), occupancy=occ.astype(np.int64), private=priv.astype(np.int64),
                    nkeys=int(nkeys.value))

    def rehash(self, keys_per_bucket: float) -> None:
        check(self._lib.pg_table_rehash(self._h, keys_per_bucket))

    def spill(self):
        """(fraction of keys outside their home line, slots per line) as of the last rehash()"""
        f, n = C.c_double(), C.c_uint32()
        check(self._lib.pg_table_spill(self._h, C.byref(f), C.byref(n)))
        return f.value, n.value

    def measure_spill(self) -> float:
        """fraction of keys outside their minimizer's home line, measured now (one pass over the table)"""
        f = C.c_double()
        check(self._lib.pg_table_measure_spill(self._h, C.byref(f)))
        return f.value

    @property
    def minimizer(self) -> int:
        """minimizer length m the table places k-mers by (0 = the k-mer itself)"""
        return int(self._lib.pg_table_minimizer(self._h))

    def set_minimizer(self, m: int) -> None:
        """pin m on an empty table (tuning knob; see include/panagram_hip.h)"""
        check(self._lib.pg_table_set_minimizer(self._h, int(m)))

    def export(self, db_idx: int) -> Tuple[np.ndarray, np.ndarray]:
        n = C.c_uint64()
        check(self._lib.pg_table_export(self._h, db_idx, None, None, 0, C.byref(n)))
        keys = np.empty(n.value, np.uint64)
        vals = np.empty(n.value, np.uint32)
        if n.value:
            check(self._lib.pg_table_export(self._h, db_idx, _ptr(keys), _ptr(vals), n.value, C.byref(n)))
        return keys, vals

    def counters_for_read(self, db_idx: int, seq) -> np.ndarray:
        """GetCountersForRead equivalent (cpp/anchor.cpp:148, index.py:934-935)."""
        v = _bytes_view(seq)
        n = max(0, len(v) - self.k + 1)
        out = np.zeros(n, np.uint32)
        check(self._lib.pg_counters_for_read(self._h, db_idx, _ptr(v), len(v), _ptr(out)))
        return out

    def anchor_contig(self, seq, colsums: bool = True):
        """One-shot: rows[nkmers,nbytes], rows100, bins[nbins,N+1], colsums[N] or None."""
        v = _bytes_view(seq)
        nk = max(0, len(v) - self.k + 1)
        binlen = 200000
        if nk // binlen < 100:
            binlen = nk // 100
        binlen = max(binlen, 1)
        nbins = (nk + binlen - 1) // binlen
        rows = np.zeros((nk, self.nbytes), np.uint8)
        rows100 = np.zeros(((nk + 99) // 100, self.nbytes), np.uint8)
        bins = np.zeros((nbins, self.ngenomes + 1), np.uint32)
        cs = np.zeros(self.ngenomes, np.uint64) if colsums else None
        nkm = C.c_uint64()
        check(self._lib.pg_anchor_contig(self._h, _ptr(v), len(v), _ptr(rows), _ptr(rows100), _ptr(bins),
                                         _ptr(cs), C.byref(nkm)))
        assert nkm.value == nk
        return rows, rows100, bins, cs

    def close(self) -> None:
        if self._h:
            self._close_children()
            self._lib.pg_table_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SCREEN_BINS = 64        # depth bins of a screen: bin c = depth c, the last = that depth and beyond
SCREEN_DEPTH_MAX = 255  # a screen's depth saturates there


class TableScreen:
    """A sample screened against a pan table (pg_screen.hip): one byte per slot of ``table`` in HBM, the depth at which the sample
    holds the slot's k-mer — the valid windows of every sequence set added whose canonical k-mer it is, both strands, saturating at
    SCREEN_DEPTH_MAX.  The table is only read.  The bytes belong to the table as it is now: after a re-hash, an insert that added
    keys, a clear or a regrow ``add`` and ``result`` raise (PG_E_INVALID) — make a new screen.  Closed before its table."""

    def __init__(self, table: "PanTable"):
        self.table, self._lib = table, table._lib
        h = C.c_void_p()
        check(self._lib.pg_screen_create(table._h, C.byref(h)))
        self._h = h
        table._adopt(self)

    def add(self, seqs: SeqSet) -> Tuple[int, int]:
        """stream ``seqs`` through the table: (its valid windows, those whose k-mer the table holds); depths accumulate over calls"""
        windows, hits = C.c_uint64(), C.c_uint64()
        check(self._lib.pg_screen_add_seqset(self._h, seqs._h, C.byref(windows), C.byref(hits)))
        return int(windows.value), int(hits.value)

    def result(self, min_count: int = 1) -> dict:
        """one pass over the table's k-mers, a k-mer SEEN when its depth is at least ``min_count`` (1 to SCREEN_DEPTH_MAX): int64
        arrays ``distinct``, ``seen``, ``private``, ``private_seen`` [genomes]; ``occ``, ``seen_occ`` [genomes + 1] by the number of
        genomes that hold a k-mer; ``depth_hist``, ``core_depth_hist`` [SCREEN_BINS] by min(depth, 63), of all k-mers and of those
        every genome holds; and ``nkeys``.  The depths stay: ask again at another ``min_count``."""
        if not 1 <= int(min_count) <= SCREEN_DEPTH_MAX:
            raise ValueError(f"min_count {min_count} (1 to {SCREEN_DEPTH_MAX})")
        n = self.table.ngenomes
        out = {name: np.zeros(size, np.uint64) for name, size in (("distinct", n), ("seen", n), ("private", n), ("private_seen", n),
                                                                  ("occ", n + 1), ("seen_occ", n + 1), ("depth_hist", SCREEN_BINS),
                                                                  ("core_depth_hist", SCREEN_BINS))}
        nkeys = C.c_uint64()
        check(self._lib.pg_screen_result(self._h, int(min_count), *[_ptr(a) for a in out.values()], C.byref(nkeys)))
        out = {name: a.astype(np.int64) for name, a in out.items()}
        out["nkeys"] = int(nkeys.value)
        return out

    def clear(self) -> None:
        """every depth back to zero: the next sample"""
        check(self._lib.pg_screen_clear(self._h))

    def close(self) -> None:
        if self._h:
            self._lib.pg_screen_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def screen_last_timing() -> dict:
    """HIP-event milliseconds of k_table_mark and k_table_screen in this thread's last ``TableScreen.add`` and ``.result``"""
    ms = (C.c_float * 2)()
    check(_lib.load().pg_screen_last_timing(ms))
    return dict(zip(("mark_ms", "screen_ms"), (float(x) for x in ms)))


NOVEL_BINS = 64  # depth bins of a novel table: bin c = depth c, the last = that depth and beyond


class NovelTable:
    """What a sample holds that a pan table does not (pg_novel.hip): a key table in HBM of the canonical k-mers of the sample's
    valid windows that ``table`` lacks, a 32-bit depth beside every key — the windows of every sequence set added, both strands,
    exact.  It starts at ``capacity_keys`` and grows on the device in front of every ``add``; the pan table is only read.  After a
    re-hash, an insert that added keys, a clear or a regrow of the pan table ``add`` raises (PG_E_INVALID) — make a new one.
    Closed before its table."""

    def __init__(self, table: "PanTable", capacity_keys: int = 1 << 20):
        self.table, self._lib = table, table._lib
        h = C.c_void_p()
        check(self._lib.pg_novel_create(table._h, int(capacity_keys), C.byref(h)))
        self._h = h
        table._adopt(self)

    def add(self, seqs: SeqSet) -> Tuple[int, int, int]:
        """stream ``seqs`` through the pan table: (its valid windows, those whose k-mer the pan table holds, the novel k-mers
        this call claimed); depths accumulate over calls"""
        windows, hits, new = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(self._lib.pg_novel_add_seqset(self._h, seqs._h, C.byref(windows), C.byref(hits), C.byref(new)))
        return int(windows.value), int(hits.value), int(new.value)

    def result(self, min_count: int = 1) -> dict:
        """one pass over the novel k-mers, a k-mer SOLID when its depth is at least ``min_count``: ``nkeys``, ``solid``,
        ``solid_windows`` (the sum of the solid depths) and the int64 array ``depth_hist`` [NOVEL_BINS] by min(depth, 63).  The
        table stays: ask again at another ``min_count``."""
        if not 1 <= int(min_count) <= 0xFFFFFFFF:
            raise ValueError(f"min_count {min_count} (1 to 2^32 - 1)")
        nkeys, solid, sw = C.c_uint64(), C.c_uint64(), C.c_uint64()
        hist = np.zeros(NOVEL_BINS, np.uint64)
        check(self._lib.pg_novel_result(self._h, int(min_count), C.byref(nkeys), C.byref(solid), C.byref(sw), _ptr(hist)))
        return {"nkeys": int(nkeys.value), "solid": int(solid.value), "solid_windows": int(sw.value), "depth_hist": hist.astype(np.int64)}

    def keys(self, min_count: int = 1, cap: Optional[int] = None):
        """(keys [uint64], depths [uint32]) of the solid k-mers, sorted by key.  ``cap`` (tests of the capacity protocol): ONE call
        with arrays of ``cap`` entries — the first of them in the table's slot order — returned behind the full number."""
        if not 1 <= int(min_count) <= 0xFFFFFFFF:
            raise ValueError(f"min_count {min_count} (1 to 2^32 - 1)")
        n = C.c_uint64()

        def call(m):
            k, d = np.zeros(m, np.uint64), np.zeros(m, np.uint32)
            check(self._lib.pg_novel_keys(self._h, int(min_count), m, _ptr(k) if m else None, _ptr(d) if m else None, C.byref(n)))
            return k, d
        if cap is not None:
            k, d = call(int(cap))
            return k, d, int(n.value)
        call(0)
        k, d = call(int(n.value))
        order = np.argsort(k, kind="stable")
        return k[order], d[order]

    def links(self, min_count: int = 1, cap: Optional[int] = None):
        """(keys [uint64], links [uint8]) of the solid k-mers, sorted by key: the link byte of a key, in its canonical orientation,
        has bit b (A C G T = 0 1 2 3) set when the k-mer that follows it with base b is solid too, bit 4 + b when the one in front
        of it with base b is (pg_unitigs.hip: k_unitig_links).  ``cap`` as ``keys`` takes it."""
        if not 1 <= int(min_count) <= 0xFFFFFFFF:
            raise ValueError(f"min_count {min_count} (1 to 2^32 - 1)")
        n = C.c_uint64()

        def call(m):
            k, l = np.zeros(m, np.uint64), np.zeros(m, np.uint8)
            check(self._lib.pg_novel_links(self._h, int(min_count), m, _ptr(k) if m else None, _ptr(l) if m else None, C.byref(n)))
            return k, l
        if cap is not None:
            k, l = call(int(cap))
            return k, l, int(n.value)
        call(0)
        k, l = call(int(n.value))
        order = np.argsort(k, kind="stable")
        return k[order], l[order]

    def unitigs(self, min_count: int = 1, cap_unitigs: Optional[int] = None, cap_bases: Optional[int] = None, fill=None) -> dict:
        """the solid k-mers compacted into unitigs — the non-branching paths of their de Bruijn graph (pg_unitigs.hip) — as arrays:
        ``offsets`` [uint64], ``kmers`` [uint32], ``depth_sum`` [uint64], ``circular`` [uint8] per unitig and ``bases`` [uint8,
        ASCII]: unitig u spells ``bases[offsets[u] : offsets[u] + kmers[u] + k - 1]``.  A linear unitig comes in one of its two
        orientations (``novel.canonical_unitig`` picks one), a circular one from its smallest k-mer on, its last k - 1 bases
        repeating its first.  Two calls: one that counts, one that fills.  ``cap_unitigs`` / ``cap_bases`` (tests of the capacity
        protocol): ONE call with arrays of that many entries, filled with the byte ``fill`` first, and ``nunitigs``, ``nbases``,
        ``ncircular`` — the full numbers — beside them."""
        if not 1 <= int(min_count) <= 0xFFFFFFFF:
            raise ValueError(f"min_count {min_count} (1 to 2^32 - 1)")
        nu, nb, nc = C.c_uint64(), C.c_uint64(), C.c_uint64()

        def call(mu, mb):
            a = {"offsets": np.zeros(mu, np.uint64), "kmers": np.zeros(mu, np.uint32), "depth_sum": np.zeros(mu, np.uint64),
                 "circular": np.zeros(mu, np.uint8), "bases": np.zeros(mb, np.uint8)}
            if fill is not None:
                for v in a.values():
                    v.view(np.uint8)[:] = int(fill)
            check(self._lib.pg_novel_unitigs(self._h, int(min_count), mu, mb, *[_ptr(a[f]) if len(a[f]) else None for f in
                                                                                   ("offsets", "kmers", "depth_sum", "circular", "bases")],
                                             C.byref(nu), C.byref(nb), C.byref(nc)))
            return a
        if cap_unitigs is not None or cap_bases is not None:
            a = call(int(cap_unitigs or 0), int(cap_bases or 0))
            a.update(nunitigs=int(nu.value), nbases=int(nb.value), ncircular=int(nc.value))
            return a
        call(0, 0)
        return call(int(nu.value), int(nb.value))

    def clean(self, min_count: int = 1, tip_kmers: Optional[int] = None, bubble_kmers: Optional[int] = None, ratio: float = 0.25,
              rounds: int = 4) -> dict:
        """error tips clipped and bubbles popped on the graph of the solid k-mers (pg_unitigs.hip: k_unitig_clean; the rule stands in
        that file's header): a dead-end branch of at most ``tip_kmers`` k-mers is dropped when a sibling at its fork is deeper by
        1 / ``ratio`` or more, the weaker of two parallel branches of at most ``bubble_kmers`` k-mers likewise (both default to
        2 k); ``rounds`` rounds at the most, each on what the round before left.  ``links`` and ``unitigs`` at the same
        ``min_count`` answer for the cleaned graph from then on; ``rounds=0``, another ``min_count``, an ``add`` or a ``clear``
        bring the raw graph back.  Returns ``clipped_tips``, ``clipped_kmers``, ``popped_bubbles``, ``popped_kmers`` and
        ``clean_rounds`` (the rounds that dropped something)."""
        if not 1 <= int(min_count) <= 0xFFFFFFFF:
            raise ValueError(f"min_count {min_count} (1 to 2^32 - 1)")
        k = int(self.table.k)
        st = (C.c_uint64 * 5)()
        check(self._lib.pg_novel_clean(self._h, int(min_count), clean_kmers(tip_kmers, k, "tip_kmers"), clean_kmers(bubble_kmers, k, "bubble_kmers"),
                                       clean_ratio_milli(ratio), clean_rounds(rounds), st))
        return dict(zip(CLEAN_STAT_NAMES, (int(x) for x in st)))

    def stats(self) -> dict:
        """``nkeys`` (the novel k-mers held), ``nslots``, ``grown`` (the times the table has grown)"""
        v = [C.c_uint64() for _ in range(3)]
        check(self._lib.pg_novel_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("nkeys", "nslots", "grown"), (int(x.value) for x in v)))

    def clear(self) -> None:
        """every k-mer gone: the next sample"""
        check(self._lib.pg_novel_clear(self._h))

    def close(self) -> None:
        if self._h:
            self._lib.pg_novel_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def novel_runs(table: "PanTable", seqs: SeqSet, cap: Optional[int] = None):
    """(run_contig, run_start, run_end [uint32], left_held, right_held [uint8], windows, novel_windows): the maximal runs of
    consecutive valid k-mer positions of the contigs of ``seqs`` whose k-mers ``table`` lacks, positions contig-relative, sorted by
    (contig, start); ``left_held`` / ``right_held``: the position in front of / behind the run is valid and its k-mer is in the
    table.  ``cap`` (tests of the capacity protocol): ONE call with arrays of ``cap`` entries, and the full number of runs behind
    the two window counts."""
    lib = table._lib
    nruns, windows, novel = C.c_uint64(), C.c_uint64(), C.c_uint64()

    def call(m):
        arrs = [np.zeros(m, np.uint32) for _ in range(3)] + [np.zeros(m, np.uint8) for _ in range(2)]
        check(lib.pg_novel_runs(table._h, seqs._h, m, *[_ptr(a) if m else None for a in arrs], C.byref(nruns), C.byref(windows), C.byref(novel)))
        return arrs
    if cap is not None:
        arrs = call(int(cap))
        return (*arrs, int(windows.value), int(novel.value), int(nruns.value))
    call(0)
    arrs = call(int(nruns.value))
    return (*arrs, int(windows.value), int(novel.value))


def novel_last_timing() -> dict:
    """HIP-event milliseconds of k_novel_count and k_novel_grow in this thread's last ``NovelTable.add``, of k_novel_scan in its last
    ``.result`` or ``.keys`` and of k_novel_runs in its last ``novel_runs``"""
    ms = (C.c_float * 4)()
    check(_lib.load().pg_novel_last_timing(ms))
    return dict(zip(("count_ms", "grow_ms", "scan_ms", "runs_ms"), (float(x) for x in ms)))


CLEAN_STAT_NAMES = ("clipped_tips", "clipped_kmers", "popped_bubbles", "popped_kmers", "clean_rounds")
CLEAN_MAX_KMERS, CLEAN_MAX_ROUNDS = 1024, 64


def clean_kmers(n: Optional[int], k: int, name: str) -> int:
    """``tip_kmers`` / ``bubble_kmers`` of ``NovelTable.clean`` checked: None is 2 k"""
    n = 2 * int(k) if n is None else int(n)
    if not 1 <= n <= CLEAN_MAX_KMERS:
        raise ValueError(f"{name} {n} (1 to {CLEAN_MAX_KMERS})")
    return n


def clean_ratio_milli(ratio: float) -> int:
    """the ratio of ``NovelTable.clean`` in per mille, rounded; ValueError unless 0 < ratio < 1 and the per mille lie in 1 to 999"""
    r = float(ratio)
    if not 0.0 < r < 1.0 or not 1 <= int(round(r * 1000)) <= 999:
        raise ValueError(f"ratio {ratio} (above 0 and below 1, in steps of 0.001)")
    return int(round(r * 1000))


def clean_rounds(rounds: int) -> int:
    if not 0 <= int(rounds) <= CLEAN_MAX_ROUNDS:
        raise ValueError(f"rounds {rounds} (0 to {CLEAN_MAX_ROUNDS})")
    return int(rounds)


def novel_clean_last_timing() -> dict:
    """HIP-event milliseconds of the k_unitig_links passes and the k_unitig_clean passes of this thread's last ``NovelTable.clean``"""
    ms = (C.c_float * 2)()
    check(_lib.load().pg_novel_clean_last_timing(ms))
    return dict(zip(("links_ms", "clean_ms"), (float(x) for x in ms)))


def novel_unitigs_last_timing() -> dict:
    """HIP-event milliseconds of k_unitig_links and of k_unitig_walk's linear and circular rounds (every pass of each; 0: not run)
    as the ``NovelTable`` of this thread's last ``.links`` or ``.unitigs`` call has summed them since its planes were built (the sums
    are the table's own): a counting call and the filling call behind it read as one; a call at another ``min_count``, or the first
    after an ``add`` or a ``clear``, starts from zero"""
    ms = (C.c_float * 3)()
    check(_lib.load().pg_novel_unitigs_last_timing(ms))
    return dict(zip(("links_ms", "walk_ms", "circular_ms"), (float(x) for x in ms)))


def homology_classes(name_lists: Sequence[Sequence[str]]) -> np.ndarray:
    """``contig_class`` for ``AnchorResult.coschedule`` from the genomes' record ids: contigs with the same id (the same
    chromosome name in different FASTAs) form one class, classes numbered in order of first appearance.  A genome
    fewer than half of whose ids occur in another genome — assemblies usually carry per-assembly accessions (CM0xxxx.1,
    another chr naming) — is paired BY POSITION instead: its i-th contig joins the class of the first genome's i-th
    contig (chromosome-level assemblies of one species list their chromosomes in the same order), so that the
    co-schedule still interleaves the genomes instead of running them one after the other.  Within an id-matched
    genome a contig whose id nobody shares (an extra scaffold) is a class of its own."""
    from collections import Counter
    occ = Counter(nm for names in name_lists for nm in set(names) if nm)
    by_id = [len(name_lists) > 1 and len(names) > 0 and 2 * sum(1 for nm in names if nm and occ[nm] > 1) >= len(names)
             for names in name_lists]
    seen, out, first = {}, [], None  # first: classes of the first genome's contigs, by position
    for g, names in enumerate(name_lists):
        mine = []
        for i, nm in enumerate(names):
            if by_id[g]:
                key = ("id", nm) if (nm and occ[nm] > 1) else ("own", g, i)
            elif first is not None and i < len(first):
                mine.append(first[i])
                continue
            else:
                key = ("own", g, i)
            mine.append(seen.setdefault(key, len(seen)))
        if first is None:
            first = mine
        out += mine
    return np.asarray(out, np.uint32)


def _windows(contigs, starts, ends, what: str):
    """contigs, starts, ends as the C ABI takes them: contiguous uint32 / uint64 / uint64, one entry per ``what``"""
    contigs = np.ascontiguousarray(contigs, np.uint32)
    starts = np.ascontiguousarray(starts, np.uint64)
    ends = np.ascontiguousarray(ends, np.uint64)
    if len(contigs) != len(starts) or len(ends) != len(starts):
        raise ValueError(f"contigs, starts and ends need one entry per {what}")
    return contigs, starts, ends


def _mask_words(ngenomes: int, given) -> np.ndarray:
    """a genome mask padded or cut to ceil(N / 32) uint32 words; None: the empty set"""
    w = np.zeros((ngenomes + 31) // 32, np.uint32)
    if given is not None:
        given = np.asarray(given, np.uint32).ravel()
        w[:min(len(w), len(given))] = given[:len(w)]
    return w


class AnchorResult:
    """Device-resident outputs of anchoring one SeqSet against one PanTable."""

    def __init__(self, table: PanTable, seqs: SeqSet, colsums: bool = True, rows_only: bool = False,
                 lowres_step: int = 100, max_bin_len: int = 200000, min_bin_count: int = 100, columns_only: bool = False):
        """``lowres_step`` / ``max_bin_len`` / ``min_bin_count``: the Python path's parameters
        (index.py:101-106, 1169-1172); the defaults are what cpp/anchor.cpp hard-codes."""
        self.table, self.seqs, self.ctx = table, seqs, table.ctx
        self.ngenomes, self.nbytes, self.lowres_step = table.ngenomes, table.nbytes, lowres_step
        self._lib = table._lib
        h = C.c_void_p()
        self.flags = (PG_ANCHOR_COLSUMS if colsums else 0) | (PG_ANCHOR_ROWS_ONLY if rows_only or columns_only else 0) | \
                     (PG_ANCHOR_COLUMNS_ONLY if columns_only else 0)
        check(self._lib.pg_result_create_ex(table._h, seqs._h, self.flags, lowres_step, max_bin_len, min_bin_count,
                                            C.byref(h)))
        self._h = h
        table._adopt(self)   # a result dies before its table and before its sequences
        seqs._adopt(self)

    @classmethod
    def rows_container(cls, ctx: Context, k: int, ngenomes: int, seqs: SeqSet, colsums: bool = True,
                       lowres_step: int = 100, max_bin_len: int = 200000, min_bin_count: int = 100) -> "AnchorResult":
        """A result without a table: ``ngenomes``-wide rows over ``seqs`` (zeroed), filled by
        ``merge_columns_range`` and finished by ``rows_epilogue`` — the writer's side of the genome-sharded mode."""
        r = cls.__new__(cls)
        r.table, r.seqs, r.ctx = None, seqs, ctx
        r.ngenomes, r.nbytes, r.lowres_step = ngenomes, (ngenomes + 7) // 8, lowres_step
        r._lib = ctx._lib
        r.flags = (PG_ANCHOR_COLSUMS if colsums else 0) | PG_ANCHOR_ROWS_ONLY
        h = C.c_void_p()
        check(r._lib.pg_result_create_rows(ctx._h, k, ngenomes, seqs._h, r.flags, lowres_step, max_bin_len,
                                           min_bin_count, C.byref(h)))
        r._h = h
        seqs._adopt(r)
        return r

    def coschedule(self, contig_group, piece_tiles: int = 0, contig_class=None) -> None:
        """Interleave the tiles of several anchor genomes (``contig_group[c]`` = genome of contig c;
        None: launch order) so that homologous regions share their table lines in L2.  ``contig_class[c]``:
        homology class of contig c (e.g. the chromosome) when the genomes list their contigs in different orders."""
        if contig_group is None:
            check(self._lib.pg_result_coschedule(self._h, None, 0))
            return
        grp = np.ascontiguousarray(contig_group, np.uint32)
        if len(grp) != len(self.seqs.lens):
            raise ValueError("contig_group needs one entry per contig")
        if contig_class is None:
            check(self._lib.pg_result_coschedule(self._h, _ptr(grp), piece_tiles))
            return
        cls = np.ascontiguousarray(contig_class, np.uint32)
        if len(cls) != len(grp):
            raise ValueError("contig_class needs one entry per contig")
        check(self._lib.pg_result_coschedule_classes(self._h, _ptr(grp), _ptr(cls), piece_tiles))


    def coschedule_ranges(self, contig_group, range_first_contig, piece_tiles: int = 0) -> None:
        """``coschedule`` with the contigs cut into consecutive ranges (starting at the given contigs, the first at 0)
        that are scheduled independently, so that ``run_range`` over whole ranges follows the schedule"""
        grp = np.ascontiguousarray(contig_group, np.uint32)
        rf = np.ascontiguousarray(range_first_contig, np.uint32)
        if len(grp) != len(self.seqs.lens):
            raise ValueError("contig_group needs one entry per contig")
        check(self._lib.pg_result_coschedule_ranges(self._h, _ptr(grp), piece_tiles, _ptr(rf), len(rf)))

    def contig_colsums(self, idx: int = 0, ncontigs: Optional[int] = None) -> np.ndarray:
        n = len(self.seqs.lens) - idx if ncontigs is None else ncontigs
        out = np.zeros((n, self.ngenomes), np.uint64)
        check(self._lib.pg_result_contig_colsums(self._h, idx, n, _ptr(out)))
        return out

    def run(self) -> None:
        """Enqueue the anchor kernels (asynchronous)."""
        check(self._lib.pg_anchor_run(self._h))

    def run_range(self, first_contig: int, ncontigs: int) -> None:
        """rows-only results: probe a contig range only (asynchronous)"""
        check(self._lib.pg_anchor_run_range(self._h, first_contig, ncontigs))

    def columns_direct(self, width: int) -> bool:
        """can ``run_columns_range`` emit ``width``-genome columns straight from the probe for this table?"""
        return bool(self._lib.pg_result_columns_direct(self._h, width))

    def run_columns_range(self, first_contig: int, ncontigs: int, width: int, dev_ptr: int) -> None:
        """probe a contig range and write its compact bit columns to ``dev_ptr`` — no rows in between (async)"""
        check(self._lib.pg_anchor_run_columns_range(self._h, first_contig, ncontigs, width, C.c_void_p(dev_ptr)))

    def timing(self):
        """(probe_ms, epilogue_ms) of the last run(), from HIP events on the context's stream."""
        a, b = C.c_float(), C.c_float()
        check(self._lib.pg_result_timing(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def timing_reset(self) -> None:
        check(self._lib.pg_result_timing_reset(self._h))

    def timing_mean(self):
        """(mean probe_ms, mean epilogue_ms, runs) over every run() since ``timing_reset()``"""
        a, b, n = C.c_double(), C.c_double(), C.c_uint32()
        check(self._lib.pg_result_timing_mean(self._h, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, int(n.value)

    def fused_runs(self) -> int:
        """whole runs of this result whose statistics were computed inside k_probe (tile by tile, from rows still in the
        cache) instead of by the pass over every row — pg_result_fused_runs; only with PG_FUSE_STATS=1 (an experiment: slower)"""
        n = C.c_uint32()
        check(self._lib.pg_result_fused_runs(self._h, C.byref(n)))
        return int(n.value)

    def rows_epilogue(self) -> None:
        """bitmap.100 / bins / column sums from the (combined) rows in the device buffer (async)."""
        check(self._lib.pg_rows_epilogue(self._h))

    def columns_bytes(self, width: int) -> int:
        return int(self._lib.pg_result_columns_bytes(self._h, width))

    def extract_columns(self, g0: int, width: int, dev_ptr: int) -> None:
        """compact bit columns of genomes [g0, g0+width) of the rows -> device buffer (async)"""
        check(self._lib.pg_result_extract_columns(self._h, g0, width, C.c_void_p(dev_ptr)))

    def merge_columns(self, dev_ptr: int, nparts: int, per: int) -> None:
        """all ranks' column blocks (block i = genomes from i*per) -> full rows (async)"""
        check(self._lib.pg_result_merge_columns(self._h, C.c_void_p(dev_ptr), nparts, per))

    def columns_bytes_range(self, width: int, first_contig: int, ncontigs: int) -> int:
        return int(self._lib.pg_result_columns_bytes_range(self._h, width, first_contig, ncontigs))

    def extract_columns_range(self, g0: int, width: int, first_contig: int, ncontigs: int, dev_ptr: int) -> None:
        check(self._lib.pg_result_extract_columns_range(self._h, g0, width, first_contig, ncontigs, C.c_void_p(dev_ptr)))

    def merge_columns_range(self, dev_ptr: int, part0: int, nparts: int, per: int, first_contig: int, ncontigs: int,
                            accumulate: bool = False, part_stride_bytes: int = 0) -> None:
        """genome blocks part0 .. part0+nparts-1 (``per`` genomes each) of a contig range -> rows (async);
        ``accumulate`` ORs them into the rows instead of writing the rows whole; ``part_stride_bytes``: distance
        between the blocks at ``dev_ptr`` (0: the range's own block size)"""
        check(self._lib.pg_result_merge_columns_range(self._h, C.c_void_p(dev_ptr), part0, nparts, per, first_contig,
                                                      ncontigs, 1 if accumulate else 0, part_stride_bytes))

    def append_columns(self, src: "AnchorResult", dev_ptr: int, nparts: int, per: int, first_contig: int = 0,
                       part_stride_bytes: int = 0) -> None:
        """``src``'s finished rows (fewer genomes; its contigs 0..n-1 are this result's from ``first_contig`` on, with the
        same k-mer counts) + ``nparts`` column blocks of ``per`` genomes at ``dev_ptr`` (the layout of
        ``extract_columns_range`` / ``run_columns_range`` over ``src``'s contigs, ``part_stride_bytes`` apart; 0: the
        block's own size) -> this result's rows, written whole in one pass (async): genome j of block i becomes bit
        ``src.ngenomes + i * per + j``.  ``rows_epilogue`` finishes them."""
        check(self._lib.pg_result_append_columns_range(self._h, first_contig, src._h, C.c_void_p(dev_ptr), nparts, per,
                                                       part_stride_bytes))

    def select_columns(self, src: "AnchorResult", sel, first_contig: int = 0) -> None:
        """``src``'s finished rows (its contigs 0..n-1 are this result's from ``first_contig`` on, with the same k-mer counts)
        -> this result's rows, written whole in one pass (async): bit j is ``src``'s bit ``sel[j]``.  ``sel``: this result's
        ``ngenomes`` distinct column numbers of ``src``, in any order.  ``rows_epilogue`` finishes them."""
        sel = np.ascontiguousarray(sel, np.uint32)
        check(self._lib.pg_result_select_columns_range(self._h, first_contig, src._h, _ptr(sel), len(sel)))

    def rows_tensor(self):
        """Zero-copy torch uint8 view of the device bitmap.1 buffer (for RCCL collectives)."""
        import torch
        (ptr, nbytes), _ = self.device_ptrs()

        class _Wrap:
            __cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 3}

        return torch.as_tensor(_Wrap(), device=torch.device("cuda", self.ctx.device))

    def contig_info(self, idx: int) -> dict:
        nk, n100 = C.c_uint64(), C.c_uint64()
        nb, bl = C.c_uint32(), C.c_uint32()
        check(self._lib.pg_result_contig_info(self._h, idx, C.byref(nk), C.byref(n100), C.byref(nb), C.byref(bl)))
        return dict(nkmers=nk.value, nrows100=n100.value, nbins=nb.value, binlen=bl.value)

    def window_stats(self, idx: int, starts, ends, step: int = 1, colsums: bool = True):
        """(hist [nwin, N+1], colsums [nwin, N] or None) of row windows [start, end) of contig idx"""
        starts = np.ascontiguousarray(starts, np.uint64)
        ends = np.ascontiguousarray(ends, np.uint64)
        n, N = len(starts), self.ngenomes
        hist = np.zeros((n, N + 1), np.uint64)
        cs = np.zeros((n, N), np.uint64) if colsums else None
        check(self._lib.pg_result_window_stats(self._h, idx, step, n, _ptr(starts), _ptr(ends), _ptr(hist), _ptr(cs)))
        return hist, cs

    def bin_colsums(self, contigs, starts, ends, step: int = 1, stride: int = 1, keep_words=None, omit_fixed: bool = False):
        """(cs [nbins, N] uint64, kept [nbins] uint64): bin i = sampled rows [starts[i], ends[i]) of contig contigs[i]'s
        bitmap.<step> rows, sampled row j = row j * stride; rows without any ``keep_words`` bit get them ORed in, and with
        ``omit_fixed`` rows whose N bits are then all set are dropped (k_bin_colsums, one launch)"""
        contigs, starts, ends = _windows(contigs, starts, ends, "bin")
        n, N = len(starts), self.ngenomes
        kw = None if keep_words is None else _mask_words(N, keep_words)  # (no mask is a null pointer, not a mask of zeros)
        cs = np.zeros((n, N), np.uint64)
        kept = np.zeros(n, np.uint64)
        check(self._lib.pg_result_bin_colsums(self._h, int(step), int(stride), n, _ptr(contigs), _ptr(starts), _ptr(ends),
                                              _ptr(kw), 1 if omit_fixed else 0, _ptr(cs), _ptr(kept)))
        return cs, kept

    def pair_counts(self, contigs, starts, ends, step: int = 1, stride: int = 1) -> np.ndarray:
        """[nwin, N, N] uint64: entry (i, a, b) = sampled rows [starts[i], ends[i]) of contig contigs[i]'s bitmap.<step> rows
        holding both genome a's and genome b's bit, sampled row j = row j * stride (k_pair_counts, one launch).  The full
        symmetric matrix; its diagonal are the column sums."""
        contigs, starts, ends = _windows(contigs, starts, ends, "window")
        n, N = len(starts), self.ngenomes
        out = np.zeros((n, N, N), np.uint64)
        check(self._lib.pg_result_pair_counts(self._h, int(step), int(stride), n, _ptr(contigs), _ptr(starts), _ptr(ends),
                                              _ptr(out)))
        return out

    def _find(self, contigs, starts, ends, have_words, lack_words, min_have, max_lack, step, stride, cap):
        """one pg_result_find_runs call -> (total, nruns [nwin], matched [nwin], run starts, run ends; the last two None
        unless 0 < total <= cap)"""
        contigs, starts, ends = _windows(contigs, starts, ends, "window")
        n = len(starts)
        if int(min_have) < 0 or int(max_lack) < 0:
            raise ValueError(f"min_have and max_lack must not be negative, got {min_have}, {max_lack}")
        masks = [_mask_words(self.ngenomes, given) for given in (have_words, lack_words)]
        nruns, matched = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        rs, re = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
        total = C.c_uint64(0)
        check(self._lib.pg_result_find_runs(self._h, int(step), int(stride), n, _ptr(contigs), _ptr(starts), _ptr(ends),
                                            _ptr(masks[0]), _ptr(masks[1]), min(int(min_have), 0xFFFFFFFF),
                                            min(int(max_lack), 0xFFFFFFFF), int(cap), _ptr(rs) if cap else None,
                                            _ptr(re) if cap else None, _ptr(nruns), _ptr(matched), C.byref(total)))
        fits = 0 < total.value <= cap
        return total.value, nruns, matched, rs[:total.value] if fits else None, re[:total.value] if fits else None

    def find_runs(self, contigs, starts, ends, have_words, lack_words, min_have, max_lack, step: int = 1, stride: int = 1):
        """(runs [total, 3] int64, matched [nwin] uint64): the maximal runs of consecutive MATCHING sampled rows of every
        window — window i = sampled rows [starts[i], ends[i]) of contig contigs[i]'s bitmap.<step> rows, sampled row
        j = row j * stride; a row matches iff popcount(row & have) >= min_have and popcount(row & lack) <= max_lack
        (``have_words`` / ``lack_words``: ceil(N / 32) words, None: the empty set).  A row of ``runs`` is (window, first
        sampled row, exclusive end), sorted by (window, start); ``matched[i]`` the matching sampled rows of window i.  The
        window's edges cut runs.  k_find_runs: a first call with room for FIND_FIRST_CAP runs, a second one only when
        there are more."""
        args = (contigs, starts, ends, have_words, lack_words, min_have, max_lack, step, stride)
        total, nruns, matched, rs, re = self._find(*args, FIND_FIRST_CAP)
        if total > FIND_FIRST_CAP:
            total, nruns, matched, rs, re = self._find(*args, total)
        runs = np.zeros((total, 3), np.int64)
        if total:
            runs[:, 0] = np.repeat(np.arange(len(nruns), dtype=np.int64), nruns.astype(np.int64))
            runs[:, 1] = rs
            runs[:, 2] = re
        return runs, matched

    def find_counts(self, contigs, starts, ends, have_words, lack_words, min_have, max_lack, step: int = 1, stride: int = 1):
        """(nruns [nwin] uint64, matched [nwin] uint64) of ``find_runs``' windows: the count launch alone (capacity 0)"""
        _, nruns, matched, _, _ = self._find(contigs, starts, ends, have_words, lack_words, min_have, max_lack, step, stride, 0)
        return nruns, matched

    def _patterns(self, contigs, starts, ends, select_words, step, stride, cap):
        """one pg_result_pattern_counts call -> (exceeded, sampled rows, keys, counts; the last two None when exceeded)"""
        contigs, starts, ends = _windows(contigs, starts, ends, "window")
        sel = None if select_words is None else _mask_words(self.ngenomes, select_words)  # (no selection is a null pointer: all)
        keys, counts = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
        nd, rows, exceeded = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
        check(self._lib.pg_result_pattern_counts(self._h, int(step), int(stride), len(starts), _ptr(contigs), _ptr(starts),
                                                 _ptr(ends), _ptr(sel), int(cap), _ptr(keys) if cap else None,
                                                 _ptr(counts) if cap else None, C.byref(nd), C.byref(rows), C.byref(exceeded)))
        if exceeded.value:
            return True, rows.value, None, None
        return False, rows.value, keys[:nd.value], counts[:nd.value]

    def pattern_counts(self, contigs, starts, ends, select_words=None, step: int = 1, stride: int = 1):
        """(keys uint64, counts uint64): the presence/absence pattern spectrum of the sampled rows of ALL windows together —
        window i = sampled rows [starts[i], ends[i]) of contig contigs[i]'s bitmap.<step> rows, sampled row j = row j * stride.
        ``select_words``: 1 to 64 genomes as ceil(N / 32) words (None: all N, which must then be at most 64); bit i of a key is
        the row's bit for the i-th selected genome in column order.  ``keys`` ascending, ``counts[i]`` the sampled rows with key
        ``keys[i]``; ``counts.sum()`` is the windows' total of sampled rows.  k_pattern_counts: a first call with room for
        PATTERN_FIRST_CAP patterns, 16 times the room per further call while the kernel reports more, ValueError beyond
        PATTERN_MAX_CAP."""
        cap = PATTERN_FIRST_CAP
        while True:
            exceeded, _, keys, counts = self._patterns(contigs, starts, ends, select_words, step, stride, cap)
            if not exceeded:
                return keys, counts
            if cap >= PATTERN_MAX_CAP:
                raise ValueError(f"more than {PATTERN_MAX_CAP} distinct patterns (the cap of pattern_counts): select fewer genomes")
            cap = min(cap * 16, PATTERN_MAX_CAP)

    def _gaps(self, contigs, starts, ends, select_words, maxlen, min_len, max_len, step, stride, cap):
        """one pg_result_absence_runs call -> (total, hist, absent, edges, nruns, genome / start / rows of the selected runs;
        the last three None unless 0 < total <= cap)"""
        contigs, starts, ends = _windows(contigs, starts, ends, "window")
        n, N = len(starts), self.ngenomes
        for name, v in (("maxlen", maxlen), ("min_len", min_len), ("max_len", max_len)):
            if not 0 <= int(v) <= 0xFFFFFFFF:
                raise ValueError(f"{name} must be a 32-bit count, got {v}")
        sel = None if select_words is None else _mask_words(N, select_words)  # (no selection is a null pointer: all)
        hist = np.zeros((n, N, int(maxlen) + 1), np.uint64)
        absent, edges, nruns = np.zeros((n, N), np.uint64), np.zeros((n, N, 2), np.uint64), np.zeros(n, np.uint64)
        rg, rs, rr = (np.zeros(cap, np.uint32) for _ in range(3))
        total = C.c_uint64(0)
        check(self._lib.pg_result_absence_runs(self._h, int(step), int(stride), n, _ptr(contigs), _ptr(starts), _ptr(ends), _ptr(sel),
                                               int(maxlen), int(min_len), int(max_len), int(cap), _ptr(rg) if cap else None,
                                               _ptr(rs) if cap else None, _ptr(rr) if cap else None, _ptr(hist), _ptr(absent),
                                               _ptr(edges), _ptr(nruns), C.byref(total)))
        t = total.value
        fits = 0 < t <= cap
        return (t, hist, absent, edges, nruns) + ((rg[:t], rs[:t], rr[:t]) if fits else (None, None, None))

    def absence_runs(self, contigs, starts, ends, select_words=None, maxlen: int = 84, min_len: int = 1, max_len: int = 0,
                     step: int = 1, stride: int = 1, emit: bool = True):
        """(runs [total, 4] int64, hist [nwin, N, maxlen + 1], absent [nwin, N], edges [nwin, N, 2]; the last three uint64):
        per genome the maximal runs of consecutive sampled rows WITHOUT its bit — window i = sampled rows [starts[i], ends[i])
        of contig contigs[i]'s bitmap.<step> rows, sampled row j = row j * stride.  A run is closed when a present row of the
        window bounds it on both sides.  ``hist[i, g, L]`` counts the closed runs of L rows (bin ``maxlen``: L >= maxlen),
        ``absent[i, g]`` the absent sampled rows, ``edges[i, g]`` the two open runs at the window's edges (both the window's
        rows when genome g holds none of them).  A row of ``runs`` is (window, genome, first sampled row, rows) of a closed
        run with min_len <= rows (and rows <= max_len unless that is 0), sorted by (window, genome, first row); with
        ``emit=False`` no run is written and ``runs`` is empty.  ``select_words``: the genomes to follow as ceil(N / 32) words
        (None: all); the others' entries are zero.  k_absence_runs: a first call with room for GAPS_FIRST_CAP runs, a second
        one only when there are more."""
        args = (contigs, starts, ends, select_words, maxlen, min_len, max_len, step, stride)
        total, hist, absent, edges, nruns, rg, rs, rr = self._gaps(*args, GAPS_FIRST_CAP if emit else 0)
        if emit and total > GAPS_FIRST_CAP:
            total, hist, absent, edges, nruns, rg, rs, rr = self._gaps(*args, total)
        runs = np.zeros((total if emit else 0, 4), np.int64)
        if emit and total:
            runs[:, 0] = np.repeat(np.arange(len(nruns), dtype=np.int64), nruns.astype(np.int64))
            runs[:, 1], runs[:, 2], runs[:, 3] = rg, rs, rr
        return runs, hist, absent, edges

    def presence_profile(self, contigs, starts, ends, select_words=None):
        """(profile [nwin, N, 6], rows [nwin, 2]; both uint32): per window and genome ``hits, runs, longest, first, end,
        covered`` of the genome's column over the window's rows — window i = rows [starts[i], ends[i]) of contig contigs[i]'s
        bitmap.1 rows.  hits: the set rows; runs: the maximal runs of set rows; longest: the rows of the longest; first / end:
        window-relative index of the first set row and one past the last (0, 0 without one); covered: the bases of the window's
        n + k - 1 that lie in at least one held k-mer (k: the result's own).  ``rows[i]``: the rows in which every selected
        genome's bit is set, and those in which none is.  ``select_words``: the genomes to follow as ceil(N / 32) words (None:
        all); the others' entries are zero, and so is everything for an empty selection or an empty window.
        k_presence_profile: one launch, one download."""
        contigs, starts, ends = _windows(contigs, starts, ends, "window")
        n, N = len(starts), self.ngenomes
        sel = None if select_words is None else _mask_words(N, select_words)  # (no selection is a null pointer: all)
        profile, rows = np.zeros((n, N, 6), np.uint32), np.zeros((n, 2), np.uint32)
        check(self._lib.pg_result_presence_profile(self._h, n, _ptr(contigs), _ptr(starts), _ptr(ends), _ptr(sel), _ptr(profile),
                                                   _ptr(rows)))
        return profile, rows

    def write_bgzf(self, step: int, gz_path: str, gzi_path: Optional[str] = None, level: int = 6,
                   threads: int = 1, first_contig: int = 0, ncontigs: Optional[int] = None) -> None:
        """Stream the bitmap.<step> payload of contigs [first_contig, first_contig + ncontigs) (default:
        all) from HBM into a BGZF file + .gzi; releases the GIL, so a worker thread can write while
        the main thread anchors on."""
        n = len(self.seqs.lens) - first_contig if ncontigs is None else ncontigs
        check(self._lib.pg_result_write_bgzf_range(self._h, step, first_contig, n, os.fsencode(gz_path),
                                                   os.fsencode(gzi_path) if gzi_path else None, level, threads))

    def inflate_bgzf(self, step: int, gz_path: str, gzi_path: Optional[str] = None, first_contig: int = 0,
                     ncontigs: Optional[int] = None, file_row0: int = 0) -> None:
        """Fill the rows of contigs [first_contig, first_contig + ncontigs) (default: all) from a bitmap.<step>.gz, inflated
        on the GPU (k_bgzf_inflate); the result's contig 0 is row ``file_row0`` of the file's payload.  Afterwards
        ``window_stats`` reads them.  A malformed block raises PanagramHipError (PG_E_FORMAT) naming its file offset."""
        n = len(self.seqs.lens) - first_contig if ncontigs is None else ncontigs
        check(self._lib.pg_result_inflate_bgzf(self._h, step, os.fsencode(gz_path), os.fsencode(gzi_path) if gzi_path else None,
                                               first_contig, n, int(file_row0)))

    @classmethod
    def from_bgzf(cls, ctx: Context, k: int, ngenomes: int, nkmers: Sequence[int], gz_path: str,
                  gzi_path: Optional[str] = None, file_row0: int = 0, step: int = 1, lowres_step: int = 100) -> "AnchorResult":
        """A rows container over contigs of ``nkmers`` rows each (contig lengths nkmers + k - 1; k - 1 for a contig without
        rows) whose bitmap.<step> rows are read back from ``gz_path`` starting at payload row ``file_row0`` (rows of that
        file: for the low-resolution bitmap, ``step`` = ``lowres_step``, the index's low-resolution step)."""
        nk = np.asarray(nkmers, np.int64)
        ss = SeqSet(ctx, np.where(nk > 0, nk + k - 1, k - 1).astype(np.uint64))
        try:
            r = cls.rows_container(ctx, k, ngenomes, ss, colsums=False, lowres_step=lowres_step)
        except Exception:
            ss.close()
            raise
        r._own_seqs = ss
        try:
            r.inflate_bgzf(step, gz_path, gzi_path, file_row0=file_row0)
        except Exception:
            r.close()
            raise
        return r

    def download(self, idx: int, want_bitmap1: bool = True, want_bitmap100: bool = True):
        info = self.contig_info(idx)
        nb = self.nbytes
        rows = np.empty((info["nkmers"], nb), np.uint8) if want_bitmap1 else None
        rows100 = np.empty((info["nrows100"], nb), np.uint8) if want_bitmap100 else None
        bins = np.empty((info["nbins"], self.ngenomes + 1), np.uint32)
        check(self._lib.pg_result_download(self._h, idx, _ptr(rows), _ptr(rows100), _ptr(bins)))
        return rows, rows100, bins, info

    def contigs_small(self, first: int = 0, ncontigs: Optional[int] = None) -> "SmallOutputs":
        """geometry and bin histograms of contigs ``first .. first+ncontigs-1`` in two library calls (one device-to-host
        copy) whatever their number — per-contig ``download`` calls cost a fragmented assembly 26 us per contig"""
        n = len(self.seqs.lens) - first if ncontigs is None else ncontigs
        nk, n100 = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        nb, bl = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        check(self._lib.pg_result_contigs_small(self._h, first, n, _ptr(nk), _ptr(n100), _ptr(nb), _ptr(bl), None, 0))
        bins = np.zeros((int(nb.sum(dtype=np.uint64)), self.ngenomes + 1), np.uint32)
        if bins.size:
            check(self._lib.pg_result_contigs_small(self._h, first, n, None, None, None, None, _ptr(bins), bins.size))
        return SmallOutputs(nk, n100, nb, bl, bins)

    def colsums(self) -> np.ndarray:
        cs = np.zeros(self.ngenomes, np.uint64)
        check(self._lib.pg_result_colsums(self._h, _ptr(cs)))
        return cs

    def device_ptrs(self):
        d1, d100 = C.c_void_p(), C.c_void_p()
        b1, b100 = C.c_uint64(), C.c_uint64()
        check(self._lib.pg_result_device_ptrs(self._h, C.byref(d1), C.byref(b1), C.byref(d100), C.byref(b100)))
        return (d1.value, b1.value), (d100.value, b100.value)

    def close(self) -> None:
        if self._h:
            self._lib.pg_result_destroy(self._h)
            self._h = None
        own = getattr(self, "_own_seqs", None)
        if own is not None:
            self._own_seqs = None
            own.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _bgzf_bsize(buf: np.ndarray, off: int) -> Optional[int]:
    """BSIZE of the BGZF block at ``off``: the BC subfield found among the gzip extra subfields (any number, any order,
    as the library's header walk reads them); None when there is none"""
    xlen = int(buf[off + 10]) | int(buf[off + 11]) << 8
    end = off + 12 + xlen
    if end > len(buf):
        return None
    i, bsize = off + 12, None
    while i + 4 <= end:
        slen = int(buf[i + 2]) | int(buf[i + 3]) << 8
        if buf[i] == ord("B") and buf[i + 1] == ord("C") and slen == 2 and i + 6 <= end:
            bsize = int(buf[i + 4]) | int(buf[i + 5]) << 8
        i += 4 + slen
    return bsize


def _bgzf_payload_bytes(buf: np.ndarray) -> int:
    """the ISIZEs of the BGZF blocks in ``buf`` summed, walking BSIZE from the first block; the walk stops at a block without
    a BC subfield"""
    total, off = 0, 0
    while off + 18 <= len(buf):
        bsize = _bgzf_bsize(buf, off)
        if bsize is None:  # (the library names the bad header)
            break
        off += bsize + 1
        total += int(buf[off - 4:off].view("<u4")[0]) if 4 <= off <= len(buf) else 0
    return total


def bgzf_inflate(ctx: Context, comp, coffs=None, roffs=None, out_bytes: Optional[int] = None) -> bytes:
    """Whole BGZF blocks held in host memory inflated on the GPU (k_bgzf_inflate) and brought back: ``coffs`` / ``roffs``
    (nblocks + 1 offsets each, ``roffs`` optional) place the blocks; without them the blocks are found from BSIZE / ISIZE.
    A malformed block raises PanagramHipError (PG_E_FORMAT) naming its offset."""
    buf = np.frombuffer(bytes(comp), np.uint8)
    co = None if coffs is None else np.ascontiguousarray(coffs, np.uint64)
    ro = None if roffs is None else np.ascontiguousarray(roffs, np.uint64)
    nblocks = 0 if co is None else len(co) - 1
    if out_bytes is None:  # (the footers' ISIZE, walked here only to size the buffer; the library walks and checks again)
        out_bytes = int(ro[-1]) if ro is not None else _bgzf_payload_bytes(buf)
    import torch  # the payload lands in a torch tensor (the library and torch share one HIP runtime) and comes home by .cpu()
    dev = torch.empty(max(16, out_bytes), dtype=torch.uint8, device=f"cuda:{ctx.device}")
    raw = C.c_uint64()
    check(ctx._lib.pg_bgzf_inflate(ctx._h, _ptr(buf), len(buf), nblocks, _ptr(co), _ptr(ro), C.c_void_p(dev.data_ptr()),
                                   out_bytes, C.byref(raw)))
    return dev[:raw.value].cpu().numpy().tobytes()


class SmallOutputs:
    """The small per-contig outputs of a run of contigs: geometry arrays and the contigs' bin rows back to back
    (``bins[nbins_total, N + 1]``).  ``out[i]`` is the tuple ``AnchorResult.download(i, False, False)`` returns."""

    def __init__(self, nkmers, nrows100, nbins, binlen, bins):
        self.nkmers, self.nrows100, self.nbins, self.binlen, self.bins = nkmers, nrows100, nbins, binlen, bins
        self.bin_off = np.concatenate([[0], np.cumsum(nbins, dtype=np.int64)])

    def __len__(self):
        return len(self.nkmers)

    def info(self, i: int) -> dict:
        return dict(nkmers=int(self.nkmers[i]), nrows100=int(self.nrows100[i]), nbins=int(self.nbins[i]), binlen=int(self.binlen[i]))

    def __getitem__(self, i: int):
        return None, None, self.bins[self.bin_off[i]:self.bin_off[i + 1]], self.info(i)

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def write_bins_tsv(self, path: str, ngenomes: int) -> None:
        """bitsum.bins.tsv of these contigs (numbered from 0), formatted by the library"""
        check(_lib.load().pg_write_bins_tsv(os.fsencode(path), ngenomes, len(self), _ptr(np.ascontiguousarray(self.nbins, np.uint32)),
                                            _ptr(np.ascontiguousarray(self.binlen, np.uint32)), _ptr(np.ascontiguousarray(self.bins, np.uint32))))


class BgzfWriter:
    """BGZF + .gzi writer (replaces htslib bgzf_* / bgzip.BGZipWriter + `bgzip -rI`)."""

    RLE = 0x100  # PG_BGZF_RLE: zlib's run-length strategy, OR-ed into level (one-byte rows)

    @staticmethod
    def ROWS(width: int) -> int:
        """PG_BGZF_ROWS(width): row-aware deflate for rows of 2..255 bytes, OR-ed into level"""
        return (width & 0xFF) << 16

    def __init__(self, path: str, level: int = 6, threads: int = 1):
        self._lib = _lib.load()
        h = C.c_void_p()
        check(self._lib.pg_bgzf_open(path.encode(), level, threads, C.byref(h)))
        self._h = h

    def write(self, data) -> None:
        v = _bytes_view(data)
        check(self._lib.pg_bgzf_write(self._h, _ptr(v), v.size))

    def close(self, gzi_path: Optional[str] = None) -> None:
        if self._h:
            h, self._h = self._h, None
            check(self._lib.pg_bgzf_close(h, gzi_path.encode() if gzi_path else None))
