"""``add``: append samples to a finished index without re-anchoring it (no reference counterpart: the reference re-runs its
whole workflow over all N + m samples to learn m new columns).

The rows of an anchor that is already in the index change in one way only: they gain one bit per added sample, and
sometimes a byte of width.  So, per old anchor A: A's FASTA is probed against a table of the NEW samples' k-mers alone (at
most 8 samples per table: the probe then emits compact bit columns, ``AnchorResult.run_columns_range``), A's old rows
come back from ``bitmap.1.gz`` batch by batch (``Genome._rows_from_disk``), and one kernel pass writes the wider rows
(``AnchorResult.append_columns``).  From there on A's files come from the code that writes them in ``Index.run``:
``rows_epilogue``, ``Genome.tabulate``, ``write_from_result``.  New anchors are anchored the ordinary way against a table of
all N + m samples.

Commit order.  Everything is written into ``<index>/.add_staging`` — itself a prepared index directory of the N + m
samples — and moved into place at the end: the anchors' files, ``kmc/``, ``config.yaml``, and ``samples.tsv`` LAST.  A failure
before that step leaves the tree byte for byte as it was (a leftover staging directory is removed by the next ``add``).
The move itself is a sequence of renames and NOT atomic for a concurrent reader: between its first rename and the rename of
``samples.tsv`` a reader sees anchors with more columns than ``samples.tsv`` names.

Limits: k <= 32; one process, one GPU; two anchors' new rows (one being written by a host thread, one being made) and one
batch of old rows must fit the free HBM; the old samples' FASTA files must still be where ``samples.tsv`` says; samples are appended at the end of the sample order;
removing or reordering samples is ``subset``'s job (subset.py: a new directory)."""
from __future__ import annotations

import logging
import os
import shutil
import time
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List

import numpy as np
import pandas as pd
import yaml

from . import engine

logger = logging.getLogger(__name__)

STAGING = ".add_staging"
GROUP = 8  # new samples per probe table: what run_columns_range takes


def _normalised_new(index, table: pd.DataFrame) -> pd.DataFrame:
    """the new samples in samples.tsv's schema, by ``Index._normalised_samples``' rules for a fresh table: the name
    regex, and a sample with a FASTA is an anchor unless the table says otherwise.  Ids continue from the index's."""
    return type(index).normalise_samples(table, None, first_id=index.ngenomes)[0]


def check(index, new: pd.DataFrame) -> None:
    """every refusal, before any file is touched"""
    from .index import is_fastq
    if not index.write_mode:
        raise ValueError("add: the index is open read-only (open it with mode='w')")
    if index.world > 1:
        raise ValueError(f"add: one process, one GPU — this run has {index.world} processes (WORLD_SIZE)")
    if len(new) == 0:
        raise ValueError("add: no new samples")
    dup = [str(n) for n in new.index if n in index.samples.index] + [str(n) for n in new.index[new.index.duplicated()]]
    if dup:
        raise ValueError("add: sample name(s) already in the index: " + ", ".join(dup))
    for name, row in new.iterrows():
        if pd.isna(row["fasta"]) or not os.path.isfile(row["fasta"]):
            raise ValueError(f"add: new sample {name!r}: no FASTA file {row['fasta']!r}")
        if bool(row["anchor"]) and is_fastq(row["fasta"]):
            raise ValueError(f"add: {name}: a FASTQ sample cannot be an anchor genome")
    if (bool(new["anchor"].any()) or any(os.path.exists(p + ".kmc_pre") for p in index.bitvec_prefixes) or
            any(os.path.exists(f) for f in (index.genome_dist_fname, index.kmer_shared_fname, index.kmer_occupancy_fname))):
        # a table of ALL samples is built (for the new anchors, to re-export kmc/bitvec*, or for kmer_shared.tsv /
        # kmer_occupancy.tsv after the commit) or every sample is sketched (genome_dist.tsv): every old sample's sequence is read
        for name, g in index.genomes.items():
            if pd.isna(g.fasta) or not os.path.isfile(g.fasta):
                raise ValueError(f"add: sample {name!r} of the index: its FASTA {g.fasta!r} is no longer there")
    for name in index.anchor_genomes:
        g = index.genomes[name]
        if pd.isna(g.fasta) or not os.path.isfile(g.fasta):
            raise ValueError(f"add: anchor {name!r} of the index: its FASTA {g.fasta!r} is no longer there")
        for f in (g.bitmap_gz_fname(1), g.chrs_fname):
            if not os.path.isfile(f):
                raise ValueError(f"add: anchor {name!r} of the index has no {os.path.basename(f)}: it was not anchored")


def _new_tables(stage, new_names: List[str]):
    """[(table, samples in it)]: the new samples' k-mers alone, GROUP samples per table (read sets by their -ci2 rule, as
    in ``Index.load_inputs``); the packed assemblies stay cached in ``stage`` for the table of all samples"""
    from .index import is_fastq, read_fastq_joined
    ctx, k = stage.context, int(stage.k)
    out = []
    for g0 in range(0, len(new_names), GROUP):
        group = new_names[g0:g0 + GROUP]
        sets = []
        for name in group:
            fasta = stage.genomes[name].fasta
            if is_fastq(fasta):
                sets.append((engine.SeqSet.from_host(ctx, [read_fastq_joined(fasta)]), 2, True))
            else:
                sets.append((stage.seqset_for(name), 1, False))
        sketch = engine.KmerSketch(ctx, k)
        for ss, _, _ in sets:
            sketch.add(ss)
        est = sketch.estimate()
        sketch.close()
        tbl = engine.PanTable(ctx, k, len(group), expected_keys=est + est // 32 + 1024, coscheduled=1)
        for j, (ss, min_count, own) in enumerate(sets):
            tbl.insert_seqset(j, ss, min_count=min_count)
            if own:
                ss.close()
        out.append((tbl, group))
    return out


def _widen_anchor(index, stage, name: str, tables, per: int, timings: Dict[str, float], keep_packed: bool = False):
    """The rows of anchor ``name`` for the N + m samples, from the old rows on disk and the new samples' columns, and their small
    outputs.  Returns (write, close): ``write()`` puts anchor/<name>/ into the staging tree (a writer thread's job: the
    bitmaps stream out of HBM while the next anchor is probed), ``close()`` frees the rows afterwards."""
    import torch
    ctx, k = index.context, int(index.k)
    old, new = index.genomes[name], stage.genomes[name]
    if old.chrs is None:
        old.load_chrs()
    ss = stage.seqset_for(name)
    chroms = list(old.chrs.index)
    sizes = [int(s) for s in old.chrs["size"]]
    if [str(c) for c in chroms] != [str(n) for n in ss.names] or sizes != [max(0, int(ln) - k + 1) for ln in ss.lens]:
        raise ValueError(f"add: {old.fasta} no longer holds the records chrs.tsv of anchor {name!r} lists")
    nparts = len(tables)
    part = dst = None
    t = time.perf_counter()

    def lap(key):
        # the breakdown tools/add_rate.py records (``index.add_breakdown``): a device synchronise per step.  Without it the steps
        # follow one another on the stream with no host wait but the one a result's close() makes, and the times are not kept.
        nonlocal t
        if not getattr(index, "add_breakdown", False):
            return
        ctx.synchronize()
        now = time.perf_counter()
        timings[key] = timings.get(key, 0.0) + now - t
        t = now
    try:
        # the new rows (and those of the anchor before, still being written), the columns and one batch of old rows have to fit
        # (the probe's result holds no rows where it emits columns itself; its one-byte rows otherwise: counted)
        dst_bytes = sum(sizes) * new.nbytes
        batches = old._annotate_batches(chroms) if chroms else []
        need = 2 * dst_bytes + sum(sizes) * (1 + nparts * per / 8.0) + max([sum(int(old.chrs.loc[c, "size"]) for c in b) * old.nbytes for b in batches] or [0])
        free = ctx.mem_info()[0]
        if need * 1.05 + (256 << 20) > free:
            raise MemoryError(f"add: anchor {name!r}: its rows of {stage.ngenomes} samples, the new columns and one batch of its old rows "
                              f"take {int(need) >> 20} MiB, the GPU has {free >> 20} MiB free")
        new.ensure_log()
        new.log.info("Appending %d sample(s) to the rows on disk", stage.ngenomes - index.ngenomes)
        dst = engine.AnchorResult.rows_container(ctx, k, stage.ngenomes, ss, colsums=True, **stage.result_geometry)
        stride = dst.columns_bytes(per)
        cols = torch.empty(max(8, stride * nparts), dtype=torch.uint8, device=torch.device("cuda", ctx.device))
        for i, (tbl, _) in enumerate(tables):  # probe: the anchor against the new samples' k-mers, columns only
            part = engine.AnchorResult(tbl, ss, colsums=False, columns_only=True)  # (no row buffer)
            if part.columns_direct(per):
                part.run_columns_range(0, len(chroms), per, cols.data_ptr() + i * stride)
            else:  # a table the probe cannot emit columns from: one-byte rows, then their columns
                part.close()
                part = engine.AnchorResult(tbl, ss, colsums=False, rows_only=True)
                part.run_range(0, len(chroms))
                part.extract_columns(0, per, cols.data_ptr() + i * stride)
            part.close()  # (waits for the probe)
            part = None
        lap("add_probe_s")
        order = {c: i for i, c in enumerate(chroms)}
        for batch in batches:
            src = old._rows_from_disk(batch)
            try:
                ctx.synchronize()
                lap("add_inflate_s")
                c0 = order[batch[0]]
                dst.append_columns(src, cols.data_ptr() + dst.columns_bytes_range(per, 0, c0), nparts, per, first_contig=c0,
                                   part_stride_bytes=stride)
                lap("add_append_s")
            finally:
                src.close()
        del cols
        dst.rows_epilogue()
        job = dict(res=dst, merged=None, genomes=[new.tabulate(dst, 0, len(chroms), [str(n) for n in ss.names])])
        lap("add_epilogue_s")
    except BaseException:
        if part is not None:
            part.close()
        if dst is not None:
            dst.close()
        stage.drop_seqset(name)
        raise

    def write():
        t0 = time.perf_counter()
        new.write_from_result(job, 0)
        timings["add_write_s"] = timings.get("add_write_s", 0.0) + time.perf_counter() - t0

    def close():
        dst.close()
        if not keep_packed:
            stage.drop_seqset(name)
    return write, close


def _finish(pending, timings) -> None:
    """wait for an anchor's writer, then free its rows"""
    fut, close = pending
    t0 = time.perf_counter()
    try:
        fut.result()
    finally:
        close()
        timings["add_write_wait_s"] = timings.get("add_write_wait_s", 0.0) + time.perf_counter() - t0


def _move_tree(src: str, dst: str) -> None:
    """every file under ``src`` renamed to its place under ``dst`` (directories made as needed)"""
    for dirpath, _, files in os.walk(src):
        to = os.path.join(dst, os.path.relpath(dirpath, src))
        os.makedirs(to, exist_ok=True)
        for f in sorted(files, key=lambda f: f == "chrs.tsv"):  # (an anchor's completion marker last)
            os.replace(os.path.join(dirpath, f), os.path.join(to, f))


def add(index, new_samples) -> List[str]:
    """``Index.add``; returns the lines the CLI prints: one per anchor rewritten and per anchor added"""
    from .index import Index
    table = pd.read_table(new_samples) if isinstance(new_samples, (str, os.PathLike)) else new_samples
    new = _normalised_new(index, table)
    check(index, new)
    n_old = index.ngenomes
    old_anchors = list(index.anchor_genomes)
    new_names = [str(n) for n in new.index]
    new_anchors = [str(n) for n in new.index[new["anchor"].astype(bool)]]
    staging = os.path.join(index.prefix, STAGING)
    shutil.rmtree(staging, ignore_errors=True)  # (what an earlier add that failed left behind)
    # a cached table describes the old samples
    if index._table is not None:
        index._table.close()
        index._table = None
    had_kmc = any(os.path.exists(p + ".kmc_pre") for p in index.bitvec_prefixes)
    derived = dict(genome_dist=os.path.exists(index.genome_dist_fname),
                   kmer_stats=os.path.exists(index.kmer_shared_fname) or os.path.exists(index.kmer_occupancy_fname),
                   annotate=[n for n in old_anchors if index.genomes[n].annotated and os.path.exists(index.genomes[n].tabix_fname("gene"))],
                   umaps=[n for n in old_anchors if os.path.exists(index.genomes[n].chrom_umaps_filename)])
    timings: Dict[str, float] = {}
    t_all = time.perf_counter()
    lines = []
    stage = None
    tables = []
    try:
        os.makedirs(staging)
        samples = pd.concat([index.samples[list(index.SAMPLE_COLUMNS)], new])
        samples.index.name = "name"
        samples.to_csv(os.path.join(staging, "samples.tsv"), sep="\t")
        prms = {k_: v for k_, v in index.params.items() if k_ != "prefix"}
        prms["anchor_genomes"] = old_anchors + new_anchors
        with open(os.path.join(staging, "config.yaml"), "w") as f:
            yaml.dump(prms, f)
        stage = Index(staging, mode="w")
        stage.device, stage.rank, stage.world = index.device, 0, 1
        stage._ctx = index.context  # (one context: the old rows are read by ``index``'s genomes, everything else by ``stage``'s)
        stage.export_kmc = had_kmc   # the exported databases are re-exported for all samples; the old ones are never loaded
        stage.kmc.use_existing = False
        stage._run_t0, stage._cpu_t0 = time.perf_counter(), time.process_time()
        # 1. the old anchors, one at a time
        if old_anchors:
            tables = _new_tables(stage, new_names)
            per = min(GROUP, len(new_names))
            with ThreadPoolExecutor(max_workers=1) as writer:
                pending = None  # (the anchor being written: at most two anchors' rows are resident)
                try:
                    for name in old_anchors:
                        # (its packed sequence stays for the table of all samples, where one is built below)
                        write, close = _widen_anchor(index, stage, name, tables, per, timings, keep_packed=bool(new_anchors or had_kmc))
                        if pending is not None:
                            _finish(pending, timings)
                        pending = (writer.submit(write), close)
                        lines.append(f"rewrote anchor {name}: {n_old} -> {stage.ngenomes} samples")
                finally:
                    if pending is not None:
                        _finish(pending, timings)
            for tbl, _ in tables:
                tbl.close()
            tables = []
        # 2. the new anchors, the ordinary way: a table of all samples (built from the new anchors' k-mers where that applies)
        if new_anchors or had_kmc:
            tbl = stage.build_table(keep=new_anchors)
            for name in new_anchors:
                stage.genomes[name].run_anchor(tbl)
                lines.append(f"added anchor {name}: {stage.ngenomes} samples")
        # 3. commit: the anchors' files first, samples.tsv last
        stage._ctx = None  # (the context is ``index``'s)
        if stage._table is not None:
            stage._table.close()
            stage._table = None
        stage.close()
        for sub in ("anchor", "kmc", "logs"):
            if os.path.isdir(os.path.join(staging, sub)):
                _move_tree(os.path.join(staging, sub), index.get_subdir(sub))
        os.replace(os.path.join(staging, "config.yaml"), index.config_fname)
        os.replace(os.path.join(staging, "samples.tsv"), index.samples_fname)
    except BaseException:
        for tbl, _ in tables:
            tbl.close()
        if stage is not None:
            stage._ctx = None
            if stage._table is not None:
                stage._table.close()
                stage._table = None
            stage.close()
        shutil.rmtree(staging, ignore_errors=True)
        raise
    shutil.rmtree(staging, ignore_errors=True)
    # the index object now describes the N + m samples
    index.anchor_genomes = old_anchors + new_anchors
    index._inputs = None
    index._minhash.clear()
    for nm in list(index._seqsets):
        index.drop_seqset(nm)
    index._load_samples()
    timings["add_total_s"] = time.perf_counter() - t_all
    index.timings.update(timings)
    # 4. derived files: refreshed by their own writers, only where they were there
    if had_kmc:
        index.write_opdefs()  # (they name the databases by path)
    if derived["kmer_stats"]:
        index.write_kmer_stats()
        index._table.close()  # (the table of every sample's k-mers: not kept beside what follows)
        index._table = None
    for name in derived["annotate"]:
        index.genomes[name].run_annotate()
    for name in derived["umaps"]:
        index.genomes[name].write_umaps()
    if derived["genome_dist"]:
        index.write_genome_dist()
    index.close()  # as ``Index.run`` leaves it: table, packed sequences and context freed, the object usable (a context comes back on demand)
    return lines
