#!/usr/bin/env python3
"""`novel --unitigs --clean` on the workload of tools/novel_unitigs_rate.py: k_unitig_links and k_unitig_clean timed with HIP events.

    python tools/novel_clean_rate.py [--genomes 8] [--mb 100] [--contigs 5] [-k 21] [--fastq-mb 1024] [--error 0.005]
                                     [--insertion 50000] [--circle 5400] [--min-count 2] [--rounds 4]

The table, the sample and the reads are those of tools/novel_unitigs_rate.py (same seeds, same defaults).  Then, at --min-count:
    raw       the unitigs of the raw graph (NovelTable.clean(rounds=0), then .unitigs): their number, N50, the longest
    rounds    NovelTable.clean(rounds=r) for r = 1 .. --rounds, each from the raw graph: the summed milliseconds of its k_unitig_links
              passes (r + 1 of them, or as many as ran) and of its k_unitig_clean passes, and what it dropped — a round's own time
              and drop are the differences between r and r - 1
    cleaned   the unitigs behind the last of them, and whether the insertion and the circle came back whole
Prints one JSON line."""
import argparse
import json
import os
import sys

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
    ap.add_argument("--min-count", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=4)
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
    sample = np.concatenate([contig[:at], ins, contig[at:], circle, circle[:149]])
    starts_end = len(sample) - 149
    k, mc = a.k, a.min_count
    nrec = max(1, int(a.fastq_mb * (1 << 20)) // record_bytes(150))
    per = max(1, int(a.batch_mb * (1 << 20)) // record_bytes(150))
    nt = engine.NovelTable(pg.table)
    for r0 in range(0, nrec, per):
        m = min(per, nrec - r0)
        s = rng.integers(0, starts_end, m)
        s = np.where((s > len(contig) + a.insertion - 150) & (s < len(contig) + a.insertion), s + 150, s)
        seqs = substituted(rng, sample[s[:, None] + np.arange(150)[None, :]], a.error)
        rs, n, used = engine.SeqSet.from_fastq(ctx, fastq_records(m, 150, a.seed + r0, seqs=seqs).reshape(-1))
        nt.add(rs)
        rs.close()
    out = dict(genomes=a.genomes, mb=a.mb, k=k, error=a.error, insertion=a.insertion, circle=a.circle, reads=nrec, min_count=mc,
               coverage=round(nrec * 150 / len(sample), 1), solid_kmers=nt.result(mc)["solid"], **nt.stats())

    def rc(s):
        return s.translate(str.maketrans("ACGT", "TGCA"))[::-1]
    ins_text, circ_text = ins.tobytes().decode(), circle.tobytes().decode()

    def unitig_report():
        u = nt.unitigs(mc)
        frame = nov.unitigs_frame(u["offsets"], u["kmers"], u["depth_sum"], u["circular"], u["bases"], k)
        whole_ins = any(ins_text in s or ins_text in rc(s) for s in frame["sequence"] if len(s) >= a.insertion)
        # how much of the insertion its longest piece holds
        best = max((len(s) for s in frame["sequence"] if len(s) >= 200 and (s[:100] in ins_text or rc(s)[:100] in ins_text)), default=0)
        circ_rows = frame[frame["circular"] == 1]
        whole_circle = any(len(s) == a.circle + k - 1 and (s[:a.circle] in circ_text * 2 or s[:a.circle] in rc(circ_text) * 2) for s in circ_rows["sequence"])
        t = engine.novel_unitigs_last_timing()
        return dict(**nov.unitig_stats(frame), nodes=int(u["kmers"].astype(np.int64).sum()), insertion_in_one_unitig=bool(whole_ins),
                    longest_piece_that_starts_in_the_insertion=int(best), circle_in_one_circular_unitig=bool(whole_circle),
                    walk_ms=round(t["walk_ms"], 3), circular_ms=round(t["circular_ms"], 3))
    nt.clean(mc, rounds=0)
    out["raw"] = unitig_report()
    out["rounds"] = []
    for r in range(1, a.rounds + 1):
        st = nt.clean(mc, rounds=r)
        t = engine.novel_clean_last_timing()
        out["rounds"].append(dict(max_rounds=r, links_ms=round(t["links_ms"], 3), clean_ms=round(t["clean_ms"], 3), **st))
        if st["clean_rounds"] < r:
            break
    out["cleaned"] = unitig_report()
    nt.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
