#!/usr/bin/env python3
"""The kernels of `screen` on inputs of real size, timed with HIP events and with the wall clock.

    python tools/screen_rate.py [--genomes 8] [--mb 100] [--contigs 5] [-k 21] [--fastq-mb 1024] [--reps 5] [--lib LIB]

A synthetic pangenome as bench.py makes it (BASELINE configs[1] by default), the table created as Index.build_table creates it.
mark     k_table_mark (engine.screen_last_timing): genome 1's packed assembly streamed through the table, the plane cleared between
         the calls; and --fastq-mb MiB of four-line FASTQ text — 150-base reads cut from genome 1 — joined on the GPU 256 MiB at a
         time (SeqSet.from_fastq) and streamed batch by batch, the kernel's times summed.  Medians of --reps calls after a warm one.
screen   k_table_screen (HIP events, and the whole call) beside PanTable.kmer_stats (k_table_pair_counts: the whole call), the two
         alternating, --reps each after a warm one.  Checked: nkeys and the distinct counts agree with kmer_stats' diagonal, and
         genome 1 as the sample is seen whole.
--lib    another build of the library (tools: build.build(out=...)) in place of the product's: the same numbers for it.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def med(v):
    v = np.asarray(v, float)
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=8)
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--contigs", type=int, default=5)
    ap.add_argument("-k", type=int, default=21)
    ap.add_argument("--d", type=float, default=0.01)
    ap.add_argument("--fastq-mb", type=float, default=1024.0)
    ap.add_argument("--batch-mb", type=float, default=256.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.lib:
        from panagram_amd import _lib
        _lib.LIB_PATH = os.path.abspath(a.lib)
    import torch
    import bench
    from panagram_amd import engine
    ctx = engine.Context(0)
    dev = torch.device("cuda:0")
    lens = [int(a.mb * 1e6) // a.contigs] * a.contigs
    pg = bench.Pangenome(ctx, dev, a.genomes, lens, a.d, 1234, a.k, keep_ascii=a.fastq_mb > 0)
    st = pg.table.stats()
    out = dict(genomes=a.genomes, mb=a.mb, k=a.k, d=a.d, reps=a.reps, lib=a.lib, table_bytes=st["bytes"], nkeys=st["nkeys"], nslots=st["nslots"],
               slots_per_line=st["nslots"] // st["nbuckets"], created_keys_per_line=pg.keys_per_line or 3, table_build_s=round(pg.build_s, 4))
    has_screen = hasattr(ctx._lib, "pg_screen_create")
    g = min(1, a.genomes - 1)
    if has_screen:
        sc = engine.TableScreen(pg.table)
        # mark: an assembly
        ms, wall = [], []
        for r in range(a.reps + 1):
            sc.clear()
            t0 = time.perf_counter()
            windows, hits = sc.add(pg.seqsets[g])
            t1 = time.perf_counter()
            if r:
                ms.append(engine.screen_last_timing()["mark_ms"])
                wall.append((t1 - t0) * 1e3)
        assert windows == hits == pg.pos_per_genome[g], (windows, hits, pg.pos_per_genome[g])
        out["mark_assembly"] = dict(windows=windows, hits=hits, mark_ms=med(ms), call_wall_ms=med(wall),
                                    g_kmers_per_s=round(windows / float(np.median(ms)) / 1e6, 2))
    # screen beside kmer_stats, alternating
    scr_ms, scr_wall, ks_wall = [], [], []
    for r in range(a.reps + 1):
        if has_screen:
            t0 = time.perf_counter()
            res = sc.result(1)
            t1 = time.perf_counter()
        t2 = time.perf_counter()
        ks = pg.table.kmer_stats()
        t3 = time.perf_counter()
        if r:
            ks_wall.append((t3 - t2) * 1e3)
            if has_screen:
                scr_ms.append(engine.screen_last_timing()["screen_ms"])
                scr_wall.append((t1 - t0) * 1e3)
    assert ks["nkeys"] == st["nkeys"]
    out["kmer_stats_call_wall_ms"] = med(ks_wall)
    if has_screen:
        assert res["nkeys"] == st["nkeys"] and res["distinct"].tolist() == np.diag(ks["pairs"]).tolist()
        assert res["occ"].tolist() == ks["occupancy"].tolist() and res["private"].tolist() == ks["private"].tolist()
        assert res["seen"][g] == res["distinct"][g] and res["private_seen"][g] == res["private"][g]
        out["screen"] = dict(screen_ms=med(scr_ms), call_wall_ms=med(scr_wall),
                             table_gb_per_s=round(st["bytes"] / float(np.median(scr_ms)) / 1e6, 1),
                             of_kmer_stats_call=round(float(np.median(scr_wall)) / float(np.median(ks_wall)), 3))
    # mark: FASTQ text
    if has_screen and a.fastq_mb > 0:
        from make_fastq import fastq_records, record_bytes
        rng = np.random.default_rng(a.seed)
        nrec = max(1, int(a.fastq_mb * (1 << 20)) // record_bytes(150))
        per = max(1, int(a.batch_mb * (1 << 20)) // record_bytes(150))
        contig = pg.ascii[g][0].cpu().numpy()
        ms, join_ms, windows, hits, nbatches = 0.0, 0.0, 0, 0, 0
        sc.clear()
        t0 = time.perf_counter()
        t_text = 0.0
        for r0 in range(0, nrec, per):
            m = min(per, nrec - r0)
            tt = time.perf_counter()
            at = rng.integers(0, len(contig) - 150, m)
            text = fastq_records(m, 150, a.seed + r0, seqs=contig[at[:, None] + np.arange(150)[None, :]]).reshape(-1)
            t_text += time.perf_counter() - tt
            rs, n, used = engine.SeqSet.from_fastq(ctx, text)
            assert n == m and used == len(text)
            join_ms += engine.place_last_timing()["fastq_ms"]
            w, h = sc.add(rs)
            rs.close()
            ms += engine.screen_last_timing()["mark_ms"]
            windows, hits, nbatches = windows + w, hits + h, nbatches + 1
        wall = time.perf_counter() - t0 - t_text
        assert windows == hits == nrec * (150 - a.k + 1)
        out["mark_fastq"] = dict(text_bytes=nrec * record_bytes(150), reads=nrec, batches=nbatches, windows=windows, hits=hits, mark_ms=round(ms, 3),
                                 g_kmers_per_s=round(windows / ms / 1e6, 2), fastq_join_ms=round(join_ms, 3),
                                 wall_s_without_making_the_text=round(wall, 3))
        res = sc.result(2)
        out["mark_fastq"]["keys_seen_at_2"] = int(res["seen_occ"].sum())
    if has_screen:
        sc.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
