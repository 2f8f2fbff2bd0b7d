#!/usr/bin/env python3
"""MinHash sketch throughput (engine.MinHashSketch: k_minhash + the host's bottom-s) in k-mers per second.

    python tools/minhash_rate.py [--mb 100] [--genomes 8] [--big-gb 3] [--reps 5] [--index-runs 2] [--skip-index]

Shapes: --genomes synthetic genomes of --mb Mb (BASELINE.json configs[1]: 8 x 100 Mb), and one --big-gb Gb genome.
Each sketch is warmed up once, then timed --reps times between two device events recorded on the library's stream
(the span holds the kernel, the candidates' download and the host's sort — add() returns when the sketch is done).
The kernel alone: run this under `rocprofv3 --kernel-trace --stats -- python tools/minhash_rate.py ...` (k_minhash).
Last, Index.run() on the --genomes x --mb case from FASTA files with and without genome_dist, alternating."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _synth  # noqa: E402
from panagram_amd import engine, index as pidx  # noqa: E402


def timed_sketch(ctx, stream, ss, distinct, reps):
    import torch
    mh = engine.MinHashSketch(ctx)
    mh.add(ss, distinct)  # warm-up
    ms = []
    for _ in range(reps):
        mh.reset()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        mh.add(ss, distinct)
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    passes = mh.passes()  # (of the last add)
    mh.close()
    return float(np.median(ms)), min(ms), passes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--genomes", type=int, default=8)
    ap.add_argument("--big-gb", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--index-runs", type=int, default=2)
    ap.add_argument("--skip-index", action="store_true")
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    ctx = engine.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    L, G = int(a.mb * 1e6), a.genomes
    gen = _synth.synth_genomes(G, [L // 5] * 5, 0.01, 1234)
    genomes = [[_synth.codes_to_ascii(c) for c in g] for g in gen]
    del gen
    total_k, total_ms = 0, 0.0
    for g in range(G):
        ss = engine.SeqSet.from_host(ctx, genomes[g])
        hll = engine.KmerSketch(ctx, 21)
        hll.add(ss)
        nk = ss.total_kmers(21)
        med, best, passes = timed_sketch(ctx, stream, ss, hll.estimate(), a.reps)
        hll.close()
        ss.close()
        total_k += nk
        total_ms += med
        print(f"genome {g}: {nk} k-mers, {med:.2f} ms median ({best:.2f} best), {nk / med / 1e6:.2f} G k-mers/s, kernel passes {passes}",
              flush=True)
    print(f"{G} x {a.mb:g} Mb: {total_k} k-mers in {total_ms:.1f} ms = {total_k / total_ms / 1e6:.2f} G k-mers/s", flush=True)
    if a.big_gb > 0:
        n = int(a.big_gb * 1e9)
        rng = np.random.default_rng(7)
        contigs = [bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n // 24, dtype=np.uint8)]) for _ in range(24)]
        ss = engine.SeqSet.from_host(ctx, contigs)
        del contigs
        hll = engine.KmerSketch(ctx, 21)
        hll.add(ss)
        nk = ss.total_kmers(21)
        med, best, passes = timed_sketch(ctx, stream, ss, hll.estimate(), a.reps)
        hll.close()
        ss.close()
        print(f"one {a.big_gb:g} Gb genome: {nk} k-mers, {med:.2f} ms median ({best:.2f} best), {nk / med / 1e6:.2f} G k-mers/s, "
              f"kernel passes {passes}", flush=True)
    ctx.close()
    if a.skip_index:
        return
    with tempfile.TemporaryDirectory() as d:
        rows = ["name\tfasta"]
        for g in range(G):
            fa = os.path.join(d, f"g{g}.fa")
            with open(fa, "wb") as f:
                f.write(_synth.fasta_text([f"chr{c + 1}" for c in range(5)], genomes[g]))
            rows.append(f"g{g}\t{fa}")
        with open(os.path.join(d, "samples.tsv"), "w") as f:
            f.write("\n".join(rows) + "\n")
        del genomes
        times = {False: [], True: []}
        for r in range(a.index_runs):
            for flag in (False, True):
                out = os.path.join(d, f"out_{r}_{int(flag)}")
                t0 = time.perf_counter()
                idx = pidx.Index(os.path.join(d, "samples.tsv"), prefix=out, k=21, genome_dist=flag)
                idx.run()
                times[flag].append(time.perf_counter() - t0)
                extra = f", load_minhash_s {idx.timings.get('load_minhash_s', 0.0):.3f}" if flag else ""
                print(f"Index.run() genome_dist={flag}: {times[flag][-1]:.2f} s{extra}", flush=True)
        print(f"Index.run() {G} x {a.mb:g} Mb median: without {np.median(times[False]):.2f} s, "
              f"with genome_dist {np.median(times[True]):.2f} s", flush=True)


if __name__ == "__main__":
    main()
