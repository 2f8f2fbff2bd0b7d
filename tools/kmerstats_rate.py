#!/usr/bin/env python3
"""Time of the pan-genome statistics pass (PanTable.kmer_stats: k_table_pair_counts) beside the table build it follows: a
synthetic pangenome as bench.py makes it, the table created as Index.build_table creates it.
   python tools/kmerstats_rate.py --genomes 8 --mb 100          (BASELINE configs[1])
   python tools/kmerstats_rate.py --genomes 128 --mb 10 --contigs 2
The streaming ceiling to hold the bytes per second against is tools/stream_bench's line A."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import bench  # noqa: E402
from panagram_amd import engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--genomes", type=int, default=8)
ap.add_argument("--mb", type=float, default=100.0)
ap.add_argument("--contigs", type=int, default=5)
ap.add_argument("--k", type=int, default=21)
ap.add_argument("--d", type=float, default=0.01)
ap.add_argument("--runs", type=int, default=5)
a = ap.parse_args()
dev = torch.device("cuda:0")
ctx = engine.Context(0)
lens = [int(a.mb * 1e6) // a.contigs] * a.contigs
pg = bench.Pangenome(ctx, dev, a.genomes, lens, a.d, 1234, a.k, keep_ascii=False)
st = pg.table.stats()
times = []
for _ in range(a.runs):
    ctx.synchronize()
    t0 = time.perf_counter()
    ks = pg.table.kmer_stats()
    times.append(time.perf_counter() - t0)
assert ks["nkeys"] == st["nkeys"] and int(ks["occupancy"].sum()) == st["nkeys"], (ks["nkeys"], st["nkeys"])
best = min(times)
print(f"{a.genomes} genomes x {a.mb:g} Mb, k={a.k}, d={a.d}: table {st['bytes'] / 1e9:.2f} GB, {st['nkeys']} keys in {st['nslots']} slots "
      f"({st['nkeys'] / st['nbuckets']:.2f} keys per line of {st['nslots'] // st['nbuckets']}), created at {pg.keys_per_line or 3:g} keys per line")
print(f"kmer_stats (call, host wall clock, best of {a.runs}): {best * 1e3:.2f} ms = {st['bytes'] / best / 1e9:.0f} GB/s of table bytes "
      f"(all runs: {', '.join(f'{t * 1e3:.2f}' for t in times)} ms)")
print(f"table_build_s {pg.build_s:.3f}: the statistics pass is {best / pg.build_s:.4f} of the build")
print(f"core {int(ks['occupancy'][-1])}, private {ks['private'].tolist()[:8]}{' ...' if a.genomes > 8 else ''}")
