#!/usr/bin/env python3
"""`subset` on inputs of real size: the select kernel beside the composition it replaces, and files to files.

    python tools/subset_rate.py [--mb 100] [--contigs 5] [--reps 7] [--genomes 9] [--no-index] [--out profiles/subset_rate.txt]

(a) kernel.  An anchor of --mb Mb in --contigs contigs, rows of random bits planted into a rows container.  At 9 -> 8,
    17 -> 16 and 65 -> 64 genomes with a middle column dropped: AnchorResult.select_columns (k_rows_select*), HIP events on
    the stream, the median of --reps calls after a warm one, and the fraction of the byte floor W_old + W_new bytes per
    position at PEAK_GBS; in the same loop, alternating, the composition that was there before: one extract_columns(g, 1)
    per kept genome into block i, then merge_columns_range(part0=0, nparts=N_new, per=1).  Both outputs are compared.
    GATE: the fused pass is not slower than the composition at any of the three shapes (exit status 1 otherwise).
    Recorded, not gated: 64 -> 8 (the even columns 0..14: the rows' second word is never fetched) and the full reversal of 16.
(b) files.  --genomes synthetic genomes of --mb Mb on disk: Index.run() of all of them, then Index.subset dropping the last
    one, beside Index.run() of the kept ones.  Recorded, not gated.
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


def shapes():
    """(label, N_old, sel, gated)"""
    def drop_middle(n):
        return [g for g in range(n) if g != n // 2]
    return [("9->8", 9, drop_middle(9), True), ("17->16", 17, drop_middle(17), True), ("65->64", 65, drop_middle(65), True),
            ("64->8", 64, list(range(0, 16, 2)), False), ("16->16 reversed", 16, list(range(16))[::-1], False)]


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
    for label, n_old, sel, gated in shapes():
        n_new = len(sel)
        wo, wn = (n_old + 7) // 8, (n_new + 7) // 8
        src = engine.AnchorResult.rows_container(ctx, k, n_old, ss, colsums=False)
        fused = engine.AnchorResult.rows_container(ctx, k, n_new, ss, colsums=False)
        comp = engine.AnchorResult.rows_container(ctx, k, n_new, ss, colsums=False)
        rows = src.rows_tensor()
        rows.copy_(torch.randint(0, 256, rows.shape, dtype=torch.uint8, device=dev))  # (stale bits and padding included: neither may count)
        block = src.columns_bytes(1)
        cols = torch.empty(block * n_new, dtype=torch.uint8, device=dev)
        # (planted rows: a merge over no contigs is what tells the library that the container holds rows)
        src.merge_columns_range(cols.data_ptr(), 0, 1, 1, 0, 0, accumulate=True)
        torch.cuda.synchronize()
        tf, tc = [], []
        for r in range(a.reps + 1):
            e[0].record()
            fused.select_columns(src, sel)
            e[1].record()
            for i, g in enumerate(sel):
                src.extract_columns(g, 1, cols.data_ptr() + i * block)
            comp.merge_columns_range(cols.data_ptr(), 0, n_new, 1, 0, a.contigs, accumulate=False)
            e[2].record()
            torch.cuda.synchronize()
            if r:
                tf.append(e[0].elapsed_time(e[1]))
                tc.append(e[1].elapsed_time(e[2]))
        same = bool(torch.equal(fused.rows_tensor(), comp.rows_tensor()))
        floor_ms = npos * (wo + wn) / (PEAK_GBS * 1e6)
        good = same and (not gated or med(tf) <= med(tc))
        line = dict(shape=label, positions=npos, fused_ms=round(med(tf), 4), fused_min_ms=round(min(tf), 4), fused_max_ms=round(max(tf), 4),
                    composed_ms=round(med(tc), 4), composed_min_ms=round(min(tc), 4), composed_max_ms=round(max(tc), 4),
                    byte_floor_ms=round(floor_ms, 4), fraction_of_floor=round(floor_ms / med(tf), 3), same_rows=same,
                    gate=("ok" if good else "FAILED") if gated or not same else "not gated")
        ok = ok and good
        say("kernel " + json.dumps(line))
        for x in (src, fused, comp):
            x.close()
        del cols, rows
        ctx.trim()
    ss.close()
    ctx.close()
    return ok


def files_leg(a, say):
    import _synth as po
    from panagram_amd import index as pidx
    G, k = a.genomes, 21
    L = int(a.mb * 1e6)
    gen = po.synth_genomes(G, [L // a.contigs] * a.contigs, 0.01, 1234)
    with tempfile.TemporaryDirectory() as d:
        rows = []
        for g in range(G):
            fa = os.path.join(d, f"g{g}.fa")
            with open(fa, "wb") as f:
                f.write(po.fasta_text([f"chr{c + 1}" for c in range(a.contigs)], [po.codes_to_ascii(c) for c in gen[g]]))
            rows.append(f"g{g}\t{fa}")
        del gen
        for nm, part in (("all", rows), ("kept", rows[:G - 1])):
            with open(os.path.join(d, f"{nm}.tsv"), "w") as f:
                f.write("name\tfasta\n" + "\n".join(part) + "\n")
        t0 = time.perf_counter()
        pidx.Index(os.path.join(d, "all.tsv"), prefix=os.path.join(d, "idx"), k=k, cores=32).run()
        t_all = time.perf_counter() - t0
        idx = pidx.Index(os.path.join(d, "idx"), mode="r", cores=32)
        t0 = time.perf_counter()
        idx.subset(os.path.join(d, "sub"), drop=[f"g{G - 1}"])
        t_sub = time.perf_counter() - t0
        parts = {k_: round(v, 3) for k_, v in idx.timings.items() if k_.startswith("subset_")}
        idx.close()
        t0 = time.perf_counter()
        pidx.Index(os.path.join(d, "kept.tsv"), prefix=os.path.join(d, "fresh"), k=k, cores=32).run()
        t_kept = time.perf_counter() - t0
    say("files " + json.dumps(dict(genomes=G, kept=G - 1, mb=a.mb, index_run_all_s=round(t_all, 2), subset_s=round(t_sub, 2),
                                   index_run_kept_s=round(t_kept, 2), subset_parts_s=parts)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--contigs", type=int, default=5)
    ap.add_argument("--genomes", type=int, default=9)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-index", action="store_true", help="the kernel leg only")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "subset_rate.txt"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least five timed repetitions")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        def say(s):
            print(s, flush=True)
            f.write(s + "\n")
            f.flush()
        say(f"# tools/subset_rate.py --mb {a.mb:g} --contigs {a.contigs} --genomes {a.genomes} --reps {a.reps}")
        ok = kernel_leg(a, say)
        if not a.no_index:
            files_leg(a, say)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
