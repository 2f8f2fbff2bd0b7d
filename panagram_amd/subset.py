"""``subset``: an index of chosen samples of a finished index, written to a new directory (no reference counterpart: to drop
or reorder samples the reference re-runs its whole workflow over the kept samples).

A row of the sub-index is the old row with some bits taken out and the rest moved: destination bit j is source bit
``sel[j]``.  So, per kept anchor A: A's old rows come back from ``bitmap.1.gz`` batch by batch (``Genome._rows_from_disk``)
and one kernel pass writes the narrower rows (``AnchorResult.select_columns``) into a rows container over contigs of the
lengths ``chrs.tsv`` lists.  From there on A's files come from the code that writes them in ``Index.run``: ``rows_epilogue``,
``Genome.tabulate``, ``write_from_result``.  No FASTA is read, no table built, nothing probed: it works on an index whose
assemblies are long gone, and nothing depends on k.

``--keep`` takes the samples in the order given (this is how columns are reordered), ``--drop`` the rest in the index's
order; ids are renumbered.  The source index is opened read-only and never touched; a failure midway removes the new
directory.  Derived files follow ``add``'s rule — refreshed by their own writers where the source has them, never created:
an annotated kept anchor needs its GFF; the UMAP files need only the new rows; ``kmc/bitvec*``, ``genome_dist.tsv``,
``kmer_shared.tsv`` and ``kmer_occupancy.tsv`` need the kept samples' sequences (``sequence_files=False``: left out).

Limits: a new directory only; one process, one GPU; two anchors' new rows (one being written by a host thread, one being
made) and one batch of old rows must fit the free HBM."""
from __future__ import annotations

import logging
import os
import shutil
import time
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import pandas as pd
import yaml

from . import engine

logger = logging.getLogger(__name__)

Names = Union[None, str, Sequence[str]]


def parse_names(arg: Names) -> Optional[List[str]]:
    """``A,B,C`` (the CLI's form) or a sequence of names -> a list; None stays None"""
    if arg is None:
        return None
    if isinstance(arg, str):
        return [s.strip() for s in arg.split(",") if s.strip()]
    return [str(s) for s in arg]


def kept_names(names: Sequence[str], keep: Names = None, drop: Names = None) -> List[str]:
    """the kept samples in their new order: ``keep`` as given, or what ``drop`` leaves in the index's order.  ValueError:
    both or neither, an unknown name, a name given twice, nothing kept."""
    names = [str(n) for n in names]
    keep, drop = parse_names(keep), parse_names(drop)
    if (keep is None) == (drop is None):
        raise ValueError("subset: give one of --keep and --drop")
    given = keep if keep is not None else drop
    unknown = [n for n in given if n not in names]
    if unknown:
        raise ValueError("subset: no such sample(s) in the index: " + ", ".join(unknown))
    twice = sorted({n for n in given if given.count(n) > 1})
    if twice:
        raise ValueError("subset: sample(s) named twice: " + ", ".join(twice))
    kept = keep if keep is not None else [n for n in names if n not in set(drop)]
    if not kept:
        raise ValueError("subset: nothing kept")
    return kept


def selection(names: Sequence[str], kept: Sequence[str]) -> np.ndarray:
    """sel[j] = the old column of new column j"""
    col = {str(n): i for i, n in enumerate(names)}
    return np.array([col[n] for n in kept], np.uint32)


def subset_samples(samples: pd.DataFrame, kept: Sequence[str], anchors: Sequence[str]) -> pd.DataFrame:
    """samples.tsv of the sub-index: the kept rows in kept order, ids 0..n-1, ``anchor`` set for the anchors it holds"""
    out = samples.loc[list(kept), [c for c in ("fasta", "gff", "id", "anchor")]].copy()
    out["id"] = np.arange(len(out), dtype=int)
    out["anchor"] = out.index.isin(list(anchors))
    out.index.name = "name"
    return out


def _sequence_files(index) -> List[str]:
    """the derived files of ``index`` that are functions of the samples' sequences, not of the rows"""
    found = [p + ".kmc_pre" for p in index.bitvec_prefixes if os.path.exists(p + ".kmc_pre")]
    return found + [f for f in (index.genome_dist_fname, index.kmer_shared_fname, index.kmer_occupancy_fname) if os.path.exists(f)]


def check(index, out_dir: str, kept: List[str], anchors: List[str], sequence_files: bool) -> None:
    """every refusal that needs the index, before ``out_dir`` is created"""
    if index.world > 1:
        raise ValueError(f"subset: one process, one GPU — this run has {index.world} processes (WORLD_SIZE)")
    src, dst = os.path.realpath(index.prefix), os.path.realpath(out_dir)
    if dst == src or dst.startswith(src + os.sep):
        raise ValueError(f"subset: {out_dir!r} is the index itself or lies inside it: in-place removal is out of scope")
    if os.path.lexists(out_dir) and (not os.path.isdir(out_dir) or os.listdir(out_dir)):
        raise ValueError(f"subset: {out_dir!r} exists and is not empty")
    for name in anchors:
        g = index.genomes[name]
        for f in (g.bitmap_gz_fname(1), g.bitmap_gzi_fname(1), g.chrs_fname):
            if not os.path.isfile(f):
                raise ValueError(f"subset: anchor {name!r} of the index has no {os.path.basename(f)}: it was not anchored")
        if g.annotated and not os.path.isfile(g.gff):
            raise ValueError(f"subset: anchor {name!r} is annotated and its GFF {g.gff!r} is no longer there")
    if sequence_files:
        derived = _sequence_files(index)
        for name in kept if derived else []:
            g = index.genomes[name]
            if pd.isna(g.fasta) or not os.path.isfile(g.fasta):
                raise ValueError(f"subset: the index has {os.path.relpath(derived[0], index.prefix)}, made from the samples' sequences, and the "
                                 f"FASTA {g.fasta!r} of sample {name!r} is no longer there (--no-sequence-files leaves such files out)")


def _narrow_anchor(index, out, name: str, sel: np.ndarray, timings: Dict[str, float]):
    """The rows of anchor ``name`` for the kept samples, from the old rows on disk, and their small outputs.  Returns
    (write, close): ``write()`` puts anchor/<name>/ into the new tree (a writer thread's job: the bitmaps stream out of HBM
    while the next anchor is made), ``close()`` frees the rows afterwards."""
    ctx, k = index.context, int(index.k)
    old, new = index.genomes[name], out.genomes[name]
    if old.chrs is None:
        old.load_chrs()
    chroms = list(old.chrs.index)
    sizes = [int(s) for s in old.chrs["size"]]
    dst = None
    t0 = time.perf_counter()
    try:
        # the new rows (and those of the anchor before, still being written) and one batch of old rows have to fit
        dst_bytes = sum(sizes) * new.nbytes
        batches = old._annotate_batches(chroms) if chroms else []
        need = 2 * dst_bytes + max([sum(int(old.chrs.loc[c, "size"]) for c in b) * old.nbytes for b in batches] or [0])
        free = ctx.mem_info()[0]
        if need * 1.05 + (256 << 20) > free:
            raise MemoryError(f"subset: anchor {name!r}: its rows of {out.ngenomes} samples and one batch of its old rows take "
                              f"{int(need) >> 20} MiB, the GPU has {free >> 20} MiB free")
        new.ensure_log()
        new.log.info("Selecting %d of %d samples out of the rows on disk", out.ngenomes, index.ngenomes)
        nk = np.asarray(sizes, np.int64)
        ss = engine.SeqSet(ctx, np.where(nk > 0, nk + k - 1, k - 1).astype(np.uint64))  # (lengths only, as AnchorResult.from_bgzf makes one)
        try:
            dst = engine.AnchorResult.rows_container(ctx, k, out.ngenomes, ss, colsums=True, **out.result_geometry)
        except Exception:
            ss.close()
            raise
        dst._own_seqs = ss
        order = {c: i for i, c in enumerate(chroms)}
        for batch in batches:
            src = old._rows_from_disk(batch)
            try:
                dst.select_columns(src, sel, first_contig=order[batch[0]])
            finally:
                src.close()  # (waits for the pass)
        dst.rows_epilogue()
        job = dict(res=dst, merged=None, genomes=[new.tabulate(dst, 0, len(chroms), [str(c) for c in chroms])])
        timings["subset_rows_s"] = timings.get("subset_rows_s", 0.0) + time.perf_counter() - t0
    except BaseException:
        if dst is not None:
            dst.close()
        raise

    def write():
        t1 = time.perf_counter()
        new.write_from_result(job, 0)
        timings["subset_write_s"] = timings.get("subset_write_s", 0.0) + time.perf_counter() - t1

    return write, dst.close


def _finish(pending) -> None:
    """wait for an anchor's writer, then free its rows"""
    fut, close = pending
    try:
        fut.result()
    finally:
        close()


def subset(index, out_dir, keep: Names = None, drop: Names = None, anchors: Names = None, sequence_files: bool = True) -> List[str]:
    """``Index.subset``; returns the lines the CLI prints: one per anchor of the source, rewritten or left behind"""
    from .index import Index
    out_dir = os.fspath(out_dir)
    kept = kept_names(index.genome_names, keep, drop)
    src_anchors = [str(n) for n in index.anchor_genomes]
    kept_anchors = [n for n in kept if n in src_anchors]
    want = parse_names(anchors)
    if want is not None:
        bad = [n for n in want if n not in kept_anchors]
        if bad:
            raise ValueError("subset: --anchors names sample(s) that are no kept anchor: " + ", ".join(bad))
        kept_anchors = [n for n in kept_anchors if n in want]
    check(index, out_dir, kept, kept_anchors, sequence_files)
    sel = selection(index.genome_names, kept)
    n_old = index.ngenomes
    had_kmc = sequence_files and any(os.path.exists(p + ".kmc_pre") for p in index.bitvec_prefixes)
    derived = dict(genome_dist=sequence_files and os.path.exists(index.genome_dist_fname),
                   kmer_stats=sequence_files and (os.path.exists(index.kmer_shared_fname) or os.path.exists(index.kmer_occupancy_fname)),
                   annotate=[n for n in kept_anchors if index.genomes[n].annotated and os.path.exists(index.genomes[n].tabix_fname("gene"))],
                   umaps=[n for n in kept_anchors if os.path.exists(index.genomes[n].chrom_umaps_filename)])
    timings: Dict[str, float] = {}
    t_all = time.perf_counter()
    out = None
    try:
        os.makedirs(out_dir, exist_ok=True)
        subset_samples(index.samples, kept, kept_anchors).to_csv(os.path.join(out_dir, "samples.tsv"), sep="\t")
        prms = {k_: v for k_, v in index.params.items() if k_ != "prefix"}
        prms["anchor_genomes"] = kept_anchors
        with open(os.path.join(out_dir, "config.yaml"), "w") as f:
            yaml.dump(prms, f)
        out = Index(out_dir, mode="w")
        out.device, out.rank, out.world = index.device, 0, 1
        out._ctx = index.context  # (one context: the old rows are read by ``index``'s genomes, everything else by ``out``'s)
        out.export_kmc = had_kmc
        out.kmc.use_existing = False
        out._run_t0, out._cpu_t0 = time.perf_counter(), time.process_time()
        with ThreadPoolExecutor(max_workers=1) as writer:
            pending = None  # (the anchor being written: at most two anchors' rows are resident)
            try:
                for name in kept_anchors:
                    write, close = _narrow_anchor(index, out, name, sel, timings)
                    if pending is not None:
                        _finish(pending)
                    pending = (writer.submit(write), close)
            finally:
                if pending is not None:
                    _finish(pending)
        timings["subset_total_s"] = time.perf_counter() - t_all
        # derived files: refreshed by their own writers, only where the source has them
        if had_kmc:
            out.build_table(keep=[])  # (exports kmc/bitvec* of the kept samples)
            out.write_opdefs()
        if derived["kmer_stats"]:
            out.write_kmer_stats()
        if out._table is not None:
            out._table.close()
            out._table = None
        for name in derived["annotate"]:
            out.genomes[name].run_annotate()
        for name in derived["umaps"]:
            out.genomes[name].write_umaps()
        if derived["genome_dist"]:
            out.write_genome_dist()
    except BaseException:
        shutil.rmtree(out_dir, ignore_errors=True)
        raise
    finally:
        if out is not None:
            out._ctx = None  # (the context is ``index``'s)
            out.close()
    index.timings.update(timings)
    index.close()  # as ``Index.add`` leaves it: context freed, the object usable (a context comes back on demand)
    return [f"rewrote anchor {n}: {n_old} -> {len(kept)} samples" if n in kept_anchors else f"dropped anchor {n}" for n in src_anchors]
