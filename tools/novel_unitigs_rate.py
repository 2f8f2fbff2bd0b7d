#!/usr/bin/env python3
"""`novel --unitigs` on inputs of real size: k_unitig_links and k_unitig_walk timed with HIP events.

    python tools/novel_unitigs_rate.py [--genomes 8] [--mb 100] [--contigs 5] [-k 21] [--fastq-mb 1024] [--error 0.005]
                                       [--insertion 50000] [--circle 5400] [--min-count 2,4]

The table of tools/novel_rate.py (a synthetic pangenome as bench.py makes it).  The sample: one contig of genome 1 carrying ONE random
insertion of --insertion bases, and a circular sequence of --circle bases; --fastq-mb MiB of four-line FASTQ text of 150-base reads
cut from it (across the circle's junction too) with substitutions at rate --error, added batch by batch to a novel table.  Then
    links     k_unitig_links over the table (NovelTable.links, counted only)
    count     the counting call of NovelTable.unitigs: the linear round's count pass — and, when a circle is there, its emit pass
              for the marks and the circular round's count pass
    fill      the filling call: the emit passes
and the unitigs, their bases, the circular ones, the longest, whether the insertion and the circle came back whole, and the time
per step of the longest unitig's walk — the count pass's time over its k-mers, an upper bound: the pass ends with its longest walk
— beside a 900-cycle HBM miss at 2.4 GHz (375 ns).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


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
    ap.add_argument("--insertion", type=int, default=50000)
    ap.add_argument("--circle", type=int, default=5400)
    ap.add_argument("--min-count", type=lambda v: [int(x) for x in v.split(",")], default=[2, 4])
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    import torch
    import bench
    from make_fastq import fastq_records, record_bytes
    from novel_rate import substituted
    from panagram_amd import engine, novel as nov
    ctx = engine.Context(0)
    dev = torch.device("cuda:0")
    lens = [int(a.mb * 1e6) // a.contigs] * a.contigs
    pg = bench.Pangenome(ctx, dev, a.genomes, lens, a.d, 1234, a.k, keep_ascii=True)
    rng = np.random.default_rng(a.seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    contig = pg.ascii[min(1, a.genomes - 1)][0].cpu().numpy()
    ins, circle = acgt[rng.integers(0, 4, a.insertion)], acgt[rng.integers(0, 4, a.circle)]
    at = len(contig) // 2
    sample = np.concatenate([contig[:at], ins, contig[at:], circle, circle[:149]])  # (reads that start in the circle may cross its junction)
    starts_end = len(sample) - 149  # a read starts anywhere but in the wrap; one that would cross from the contig into the circle starts in the circle
    k = a.k
    out = dict(genomes=a.genomes, mb=a.mb, k=k, error=a.error, insertion=a.insertion, circle=a.circle,
               sample_bases=int(len(sample)) - 149)
    nrec = max(1, int(a.fastq_mb * (1 << 20)) // record_bytes(150))
    per = max(1, int(a.batch_mb * (1 << 20)) // record_bytes(150))
    nt = engine.NovelTable(pg.table)
    count_ms = 0.0
    for r0 in range(0, nrec, per):
        m = min(per, nrec - r0)
        s = rng.integers(0, starts_end, m)
        s = np.where((s > len(contig) + a.insertion - 150) & (s < len(contig) + a.insertion), s + 150, s)
        seqs = substituted(rng, sample[s[:, None] + np.arange(150)[None, :]], a.error)
        rs, n, used = engine.SeqSet.from_fastq(ctx, fastq_records(m, 150, a.seed + r0, seqs=seqs).reshape(-1))
        nt.add(rs)
        rs.close()
        count_ms += engine.novel_last_timing()["count_ms"]
    out.update(reads=nrec, text_bytes=nrec * record_bytes(150), coverage=round(nrec * 150 / len(sample), 1), novel_count_ms=round(count_ms, 2),
               novel_kmers=nt.stats()["nkeys"], **nt.stats())
    out["unitigs"] = {}

    def rc(s):
        return s.translate(str.maketrans("ACGT", "TGCA"))[::-1]
    ins_text, circ_text = ins.tobytes().decode(), circle.tobytes().decode()
    for mc in a.min_count:
        res = nt.result(mc)
        t0 = time.perf_counter()
        nlinks = nt.links(mc, cap=0)[2]
        t1 = time.perf_counter()
        links_ms = engine.novel_unitigs_last_timing()["links_ms"]
        counted = nt.unitigs(mc, cap_unitigs=0, cap_bases=0)
        t2 = time.perf_counter()
        tc = engine.novel_unitigs_last_timing()
        u = nt.unitigs(mc)
        t3 = time.perf_counter()
        tf = engine.novel_unitigs_last_timing()  # (the times go on adding up while the planes are kept: the filling calls' are the difference)
        assert nlinks == res["solid"] and counted["nunitigs"] == len(u["kmers"]) and counted["nbases"] == len(u["bases"])
        frame = nov.unitigs_frame(u["offsets"], u["kmers"], u["depth_sum"], u["circular"], u["bases"], k)
        passes = 2 if counted["ncircular"] else 1  # (with a circle the linear emit pass runs for the marks)
        longest = int(u["kmers"].max()) if len(u["kmers"]) else 0
        whole_ins = any(ins_text in s or ins_text in rc(s) for s in frame["sequence"] if len(s) >= a.insertion)
        circ_rows = frame[frame["circular"] == 1]
        whole_circle = any(len(s) == a.circle + k - 1 and (s[:a.circle] in circ_text * 2 or s[:a.circle] in rc(circ_text) * 2) for s in circ_rows["sequence"])
        out["unitigs"][mc] = dict(solid_kmers=res["solid"], links_ms=round(links_ms, 3), links_call_wall_ms=round((t1 - t0) * 1e3, 2),
                              count_walk_ms=round(tc["walk_ms"], 3), count_circular_ms=round(tc["circular_ms"], 3), count_call_wall_ms=round((t2 - t1) * 1e3, 2),
                              fill_walk_ms=round(tf["walk_ms"] - tc["walk_ms"], 3), fill_circular_ms=round(tf["circular_ms"] - tc["circular_ms"], 3),
                              fill_calls_wall_ms=round((t3 - t2) * 1e3, 2), **nov.unitig_stats(frame), longest_kmers=longest,
                              walk_passes_in_count=passes, ns_per_step_of_the_longest_walk=round(tc["walk_ms"] * 1e6 / passes / max(longest, 1), 1), hbm_miss_ns_at_900_cycles=375,
                              insertion_in_one_unitig=bool(whole_ins), circular_kmers=circ_rows["kmers"].tolist()[:8],
                              circle_in_one_circular_unitig=bool(whole_circle),
                              mean_depth_of_the_longest=float(frame["depth"].iloc[0]) if len(frame) else 0.0)
    nt.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
