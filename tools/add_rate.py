#!/usr/bin/env python3
"""`add` on inputs of real size: the append kernel beside the path it replaces, and files to files.

    python tools/add_rate.py [--mb 100] [--contigs 5] [--reps 7] [--genomes 8] [--no-index] [--out profiles/add_rate.txt]

(a) kernel.  An anchor of --mb Mb in --contigs contigs, rows of random bits planted into rows containers, one random column
    block of one genome.  At 8 -> 9, 16 -> 17 and 64 -> 65 genomes: AnchorResult.append_columns (k_rows_append<NW>), HIP
    events on the stream, the median of --reps calls after a warm one, and the fraction of the byte floor W_old + W_new +
    1 / 8 bytes per position at PEAK_GBS; in the same loop, alternating, the composition that was there before:
    extract_columns(0, N_old) of the old rows, merge_columns_range of those columns into the new rows, then
    merge_columns_range(accumulate) of the new genome's block.  Both outputs are compared.
    GATE: the fused pass is not slower than the composition at any of the three shapes (exit status 1 otherwise).
(b) files.  --genomes + 1 synthetic genomes of --mb Mb on disk: Index.run() of the first --genomes, then Index.add of the
    last one — once as a user runs it, once (from a copy of the same tree) with Index.add_breakdown: probe, inflate, append,
    epilogue, write, a host clock around device synchronises — beside Index.run() of all of them.  Recorded, not gated.
Appends what it prints to --out."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

PEAK_GBS = 8000.0  # HBM3E of an MI355X, GB/s


def med(v):
    return float(np.median(np.asarray(v, float)))


def kernel_leg(a, say):
    import torch
    from panagram_amd import engine
    ctx = engine.Context(0)
    ctx.set_stream(0)  # torch's stream: its events time the library's launches
    dev = torch.device("cuda:0")
    k = 21
    nk = int(a.mb * 1e6) // a.contigs
    ss = engine.SeqSet(ctx, [nk + k - 1] * a.contigs)
    npos = nk * a.contigs
    ok = True
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for n_old, n_new in ((8, 9), (16, 17), (64, 65)):
        wo, wn = (n_old + 7) // 8, (n_new + 7) // 8
        src = engine.AnchorResult.rows_container(ctx, k, n_old, ss, colsums=False)
        fused = engine.AnchorResult.rows_container(ctx, k, n_new, ss, colsums=False)
        comp = engine.AnchorResult.rows_container(ctx, k, n_new, ss, colsums=False)
        rows = src.rows_tensor()
        rows.copy_(torch.randint(0, 256, rows.shape, dtype=torch.uint8, device=dev))
        # the new genome's column: random bits, none past a contig's end (what the probe writes)
        want = torch.randint(0, 2, (a.contigs, nk), dtype=torch.uint8, device=dev)
        one = engine.AnchorResult.rows_container(ctx, k, 1, ss, colsums=False)
        r1 = one.rows_tensor()
        r1.zero_()
        stride1 = (nk + 15) & ~15
        for c in range(a.contigs):
            r1[c * stride1:c * stride1 + nk] = want[c]
        col = torch.empty(one.columns_bytes(1), dtype=torch.uint8, device=dev)
        # (planted rows: a merge over no contigs is what tells the library that the containers hold rows)
        one.merge_columns_range(col.data_ptr(), 0, 1, 1, 0, 0, accumulate=True)
        src.merge_columns_range(col.data_ptr(), 0, 1, 1, 0, 0, accumulate=True)
        one.extract_columns(0, 1, col.data_ptr())
        torch.cuda.synchronize()
        one.close()
        del want, r1
        oldcols = torch.empty(src.columns_bytes(n_old), dtype=torch.uint8, device=dev)
        tf, tc = [], []
        for r in range(a.reps + 1):
            e[0].record()
            fused.append_columns(src, col.data_ptr(), 1, 1)
            e[1].record()
            src.extract_columns(0, n_old, oldcols.data_ptr())
            comp.merge_columns_range(oldcols.data_ptr(), 0, 1, n_old, 0, a.contigs, accumulate=False)
            comp.merge_columns_range(col.data_ptr(), n_old, 1, 1, 0, a.contigs, accumulate=True)
            e[2].record()
            torch.cuda.synchronize()
            if r:
                tf.append(e[0].elapsed_time(e[1]))
                tc.append(e[1].elapsed_time(e[2]))
        same = bool(torch.equal(fused.rows_tensor(), comp.rows_tensor()))
        floor_ms = npos * (wo + wn + 1 / 8) / (PEAK_GBS * 1e6)
        line = dict(shape=f"{n_old}->{n_new}", positions=npos, fused_ms=round(med(tf), 4), fused_min_ms=round(min(tf), 4), fused_max_ms=round(max(tf), 4),
                    composed_ms=round(med(tc), 4), composed_min_ms=round(min(tc), 4), composed_max_ms=round(max(tc), 4),
                    byte_floor_ms=round(floor_ms, 4), fraction_of_floor=round(floor_ms / med(tf), 3), same_rows=same,
                    gate="ok" if med(tf) <= med(tc) and same else "FAILED")
        ok = ok and line["gate"] == "ok"
        say("kernel " + json.dumps(line))
        for x in (src, fused, comp):
            x.close()
        del oldcols, col, rows
        ctx.trim()
    ss.close()
    ctx.close()
    return ok


def files_leg(a, say):
    import _synth as po
    from panagram_amd import index as pidx
    G, k = a.genomes, 21
    L = int(a.mb * 1e6)
    gen = po.synth_genomes(G + 1, [L // a.contigs] * a.contigs, 0.01, 1234)
    with tempfile.TemporaryDirectory() as d:
        rows = []
        for g in range(G + 1):
            fa = os.path.join(d, f"g{g}.fa")
            with open(fa, "wb") as f:
                f.write(po.fasta_text([f"chr{c + 1}" for c in range(a.contigs)], [po.codes_to_ascii(c) for c in gen[g]]))
            rows.append(f"g{g}\t{fa}")
        del gen
        for nm, part in (("old", rows[:G]), ("new", rows[G:]), ("all", rows)):
            with open(os.path.join(d, f"{nm}.tsv"), "w") as f:
                f.write("name\tfasta\n" + "\n".join(part) + "\n")
        t0 = time.perf_counter()
        pidx.Index(os.path.join(d, "old.tsv"), prefix=os.path.join(d, "idx"), k=k, cores=32).run()
        t_old = time.perf_counter() - t0
        # twice from the same old tree: as a user runs it, and with the breakdown's synchronises
        import shutil
        shutil.copytree(os.path.join(d, "idx"), os.path.join(d, "idx2"))
        idx = pidx.Index(os.path.join(d, "idx2"), mode="w", cores=32)
        t0 = time.perf_counter()
        idx.add(os.path.join(d, "new.tsv"))
        t_plain = time.perf_counter() - t0
        idx.close()
        idx = pidx.Index(os.path.join(d, "idx"), mode="w", cores=32)
        idx.add_breakdown = True
        t0 = time.perf_counter()
        idx.add(os.path.join(d, "new.tsv"))
        t_add = time.perf_counter() - t0
        parts = {k_: round(v, 3) for k_, v in idx.timings.items() if k_.startswith("add_")}
        idx.close()
        t0 = time.perf_counter()
        pidx.Index(os.path.join(d, "all.tsv"), prefix=os.path.join(d, "fresh"), k=k, cores=32).run()
        t_all = time.perf_counter() - t0
    say("files " + json.dumps(dict(genomes=G, mb=a.mb, index_run_old_s=round(t_old, 2), add_one_s=round(t_plain, 2), add_one_with_breakdown_s=round(t_add, 2),
                                   index_run_all_s=round(t_all, 2), add_breakdown_s=parts)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--contigs", type=int, default=5)
    ap.add_argument("--genomes", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-index", action="store_true", help="the kernel leg only")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "add_rate.txt"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least five timed repetitions")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        def say(s):
            print(s, flush=True)
            f.write(s + "\n")
            f.flush()
        say(f"# tools/add_rate.py --mb {a.mb:g} --contigs {a.contigs} --genomes {a.genomes} --reps {a.reps}")
        ok = kernel_leg(a, say)
        if not a.no_index:
            files_leg(a, say)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
