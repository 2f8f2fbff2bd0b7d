#!/usr/bin/env python3
"""The kernels of `novel` on inputs of real size, timed with HIP events and with the wall clock.

    python tools/novel_rate.py [--genomes 8] [--mb 100] [--contigs 5] [-k 21] [--fastq-mb 1024] [--error 0.005] [--reps 5] [--lib LIB]

A synthetic pangenome as bench.py makes it (BASELINE configs[1] by default), the table created as Index.build_table creates it —
the table tools/screen_rate.py builds.
count    k_novel_count (engine.novel_last_timing) beside k_table_mark (engine.screen_last_timing), the two alternating: genome 1's
         packed assembly, every window a hit, so no key is claimed and the two share the probe; the screen's plane and the novel
         table cleared between the calls.  Medians of --reps calls after a warm one.
fastq    --fastq-mb MiB of four-line FASTQ text — 150-base reads cut from genome 1 with substitutions at rate --error — joined on
         the GPU 256 MiB at a time and added batch by batch to a novel table created for 2^20 keys: k_novel_count's times summed,
         and per batch the growth step in front of it (the slots before and after, k_novel_grow's time).  The claims are mostly
         keys of depth 1: the worst case.
scan     k_novel_scan's count pass over that table beside a reduction that streams 12 bytes per slot (torch.sum over as many
         bytes); keys() with both passes.
runs     k_novel_runs (both passes) on genome 1's assembly — no run — and on one contig of it with substitutions at --error.
--lib    another build of the library (build.build(out=..., defines=["PG_NOVEL_SCAN_BLOCKS=524288"], only=["pg_novel.hip",
         "pg_api_novel.hip"]): one block of k_novel_scan per 4096 slots) in place of the product's: the same numbers for it.
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


def substituted(rng, ascii_arr, rate):
    """uint8 ASCII of any shape with substitutions at ``rate`` (the new base differs)"""
    out = ascii_arr.copy()
    hit = np.flatnonzero(rng.random(out.size) < rate)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    flat = out.reshape(-1)
    code = np.searchsorted(acgt, flat[hit])
    flat[hit] = acgt[(code + rng.integers(1, 4, len(hit))) % 4]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=8)
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--contigs", type=int, default=5)
    ap.add_argument("-k", type=int, default=21)
    ap.add_argument("--d", type=float, default=0.01)
    ap.add_argument("--fastq-mb", type=float, default=1024.0)
    ap.add_argument("--batch-mb", type=float, default=256.0)
    ap.add_argument("--error", type=float, default=0.005)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.lib:
        from panagram_amd import _lib
        _lib.LIB_PATH = os.path.abspath(a.lib)
    import torch
    import bench
    from make_fastq import fastq_records, record_bytes
    from panagram_amd import engine
    ctx = engine.Context(0)
    dev = torch.device("cuda:0")
    lens = [int(a.mb * 1e6) // a.contigs] * a.contigs
    pg = bench.Pangenome(ctx, dev, a.genomes, lens, a.d, 1234, a.k, keep_ascii=True)
    st = pg.table.stats()
    out = dict(genomes=a.genomes, mb=a.mb, k=a.k, d=a.d, error=a.error, reps=a.reps, lib=a.lib, table_bytes=st["bytes"], nkeys=st["nkeys"], nslots=st["nslots"],
               slots_per_line=st["nslots"] // st["nbuckets"])
    g = min(1, a.genomes - 1)
    rng = np.random.default_rng(a.seed)

    # count beside mark: an assembly of an indexed genome
    sc = engine.TableScreen(pg.table)
    nt = engine.NovelTable(pg.table)
    cms, mms, cwall, mwall = [], [], [], []
    for r in range(a.reps + 1):
        sc.clear()
        nt.clear()
        t0 = time.perf_counter()
        windows, hits = sc.add(pg.seqsets[g])
        t1 = time.perf_counter()
        nw, nh, new = nt.add(pg.seqsets[g])
        t2 = time.perf_counter()
        if r:
            mms.append(engine.screen_last_timing()["mark_ms"])
            cms.append(engine.novel_last_timing()["count_ms"])
            mwall.append((t1 - t0) * 1e3)
            cwall.append((t2 - t1) * 1e3)
    assert (nw, nh, new) == (windows, hits, 0) and windows == hits == pg.pos_per_genome[g]
    out["count_assembly"] = dict(windows=windows, count_ms=med(cms), mark_ms=med(mms), count_call_wall_ms=med(cwall), mark_call_wall_ms=med(mwall),
                                 count_g_kmers_per_s=round(windows / float(np.median(cms)) / 1e6, 2),
                                 mark_g_kmers_per_s=round(windows / float(np.median(mms)) / 1e6, 2), novel_slots=nt.stats()["nslots"])
    sc.close()
    nt.close()

    # runs on the same assembly, and on one contig with substitutions
    rms = []
    for r in range(a.reps + 1):
        res = engine.novel_runs(pg.table, pg.seqsets[g])
        if r:
            rms.append(engine.novel_last_timing()["runs_ms"])
    assert len(res[0]) == 0 and res[5] == windows and res[6] == 0
    out["runs_assembly"] = dict(windows=windows, runs=0, runs_ms=med(rms), g_kmers_per_s=round(windows / float(np.median(rms)) / 1e6, 2))
    contig = pg.ascii[g][0].cpu().numpy()
    ss = engine.SeqSet.from_host(ctx, [substituted(rng, contig, a.error)])
    rms = []
    for r in range(a.reps + 1):
        res = engine.novel_runs(pg.table, ss)
        if r:
            rms.append(engine.novel_last_timing()["runs_ms"])
    ss.close()
    out["runs_substituted_contig"] = dict(windows=res[5], novel_windows=res[6], runs=len(res[0]), runs_ms=med(rms),
                                          g_kmers_per_s=round(res[5] / float(np.median(rms)) / 1e6, 2))

    # FASTQ text with errors: the growth steps, the counts
    if a.fastq_mb > 0:
        nrec = max(1, int(a.fastq_mb * (1 << 20)) // record_bytes(150))
        per = max(1, int(a.batch_mb * (1 << 20)) // record_bytes(150))
        nt = engine.NovelTable(pg.table)
        steps, ms, windows, hits = [], 0.0, 0, 0
        t_text, t0 = 0.0, time.perf_counter()
        for r0 in range(0, nrec, per):
            m = min(per, nrec - r0)
            tt = time.perf_counter()
            at = rng.integers(0, len(contig) - 150, m)
            seqs = substituted(rng, contig[at[:, None] + np.arange(150)[None, :]], a.error)
            text = fastq_records(m, 150, a.seed + r0, seqs=seqs).reshape(-1)
            t_text += time.perf_counter() - tt
            rs, n, used = engine.SeqSet.from_fastq(ctx, text)
            assert n == m and used == len(text)
            before = nt.stats()
            tw = time.perf_counter()
            w, h, new = nt.add(rs)
            call_ms = (time.perf_counter() - tw) * 1e3
            rs.close()
            t = engine.novel_last_timing()
            after = nt.stats()
            ms += t["count_ms"]
            windows, hits = windows + w, hits + h
            steps.append(dict(windows=w, hits=h, new_keys=new, count_ms=round(t["count_ms"], 3), g_kmers_per_s=round(w / t["count_ms"] / 1e6, 2),
                              slots_before=before["nslots"], slots_after=after["nslots"], keys_before=before["nkeys"],
                              grow_ms=round(t["grow_ms"], 3), add_call_wall_ms=round(call_ms, 2)))
        wall = time.perf_counter() - t0 - t_text
        out["count_fastq"] = dict(text_bytes=nrec * record_bytes(150), reads=nrec, windows=windows, hits=hits, novel_windows=windows - hits,
                                  count_ms=round(ms, 3), g_kmers_per_s=round(windows / ms / 1e6, 2), batches=steps,
                                  wall_s_without_making_the_text=round(wall, 3), **nt.stats())
        # scan beside a reduction over 12 bytes per slot
        nslots = nt.stats()["nslots"]
        buf = torch.zeros(12 * nslots // 8, dtype=torch.int64, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sms, swall, tms, kms = [], [], [], []
        for r in range(a.reps + 1):
            t0 = time.perf_counter()
            res = nt.result(2)
            t1 = time.perf_counter()
            e0.record()
            buf.sum()
            e1.record()
            torch.cuda.synchronize()
            if r:
                sms.append(engine.novel_last_timing()["scan_ms"])
                swall.append((t1 - t0) * 1e3)
                tms.append(e0.elapsed_time(e1))
        del buf
        for r in range(3):
            keys, depths = nt.keys(2)
            kms.append(engine.novel_last_timing()["scan_ms"])
        assert res["nkeys"] == nt.stats()["nkeys"] and len(keys) == res["solid"] and int(depths.sum()) == res["solid_windows"]
        out["scan"] = dict(nslots=nslots, table_bytes=12 * nslots, nkeys=res["nkeys"], solid_at_2=res["solid"], solid_windows=res["solid_windows"],
                           depth_hist_1_to_4=res["depth_hist"][1:5].tolist(), scan_ms=med(sms), call_wall_ms=med(swall), stream_12_bytes_per_slot_ms=med(tms),
                           gb_per_s=round(12 * nslots / float(np.median(sms)) / 1e6, 1), keys_both_passes_ms=med(kms[1:]))
        nt.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
