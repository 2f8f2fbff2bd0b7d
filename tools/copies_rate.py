"""The copy-number kernels on genomes of real size: k_copy_insert, k_copy_count and k_copy_profile, timed with HIP events.

    python tools/copies_rate.py [--mb 100] [--contigs 5] [-k 21] [--reps 5] [--lib PATH]

A synthetic genome of --mb megabases in --contigs chromosomes, i.i.d. uniform, drawn with torch on the GPU and packed there
(SeqSet.load_dev), and three target sets:
  genes       --genes pieces of --gene-len bases cut from the genome: almost no window of the genome hits
  chromosome  the genome's first chromosome as the target, and that chromosome streamed: every window hits, each its own counter
  repeats     a second genome in which every fifth stretch of 10 kb is a homopolymer or a satellite of period 2, 3 or 5, the
              targets those repeats' k-mers: a fifth of the windows hit, all of them a handful of counters — 64 lanes of a wave on one
Per set the three kernels' times (engine.copies_last_timing: the median of --reps calls after a warm one, the spread beside it),
k_copy_count's positions per second, and two figures beside it: the streaming floor — the packed genome is 0.375 byte per
position (2 bits of sequence, 1 bit of mask), read once — at --hbm-gbs, and k_pos_mates' rate on the same sequences and box
(engine.synteny_last_timing of the streamed set against itself): the same walk with one probe and one store per position.
Checked at this size: hits equal the sum of the depths over the distinct target keys where that is known by construction.
--lib: another build of the library (python -m panagram_amd.build --out=... --csrc=... --only=pg_copies.hip) for an A/B on one
box — how the three ways to add equal slots of a wave were compared (profiles/copies_rate.txt).  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def packed(ctx, engine, codes):
    """a SeqSet of the torch uint8 code tensors (0..3) in ``codes``"""
    import torch
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=codes[0].device)
    ss = engine.SeqSet(ctx, [int(c.numel()) for c in codes])
    for i, c in enumerate(codes):
        t = acgt[c.long()]
        torch.cuda.synchronize()
        ss.load_dev(i, t.data_ptr(), int(t.numel()))
        ctx.synchronize()
    return ss


def with_repeats(c, gen, stretch=10_000):
    """every fifth stretch of ``c`` overwritten by a repeat of period 1, 2, 3 or 5 in turn"""
    import torch
    units = [[0], [0, 1], [0, 1, 2], [0, 1, 2, 3, 1]]
    c = c.clone()
    for j, s in enumerate(range(0, int(c.numel()) - stretch, 5 * stretch)):
        u = torch.tensor(units[j % 4], dtype=torch.uint8, device=c.device)
        c[s:s + stretch] = u.repeat(stretch // len(u) + 1)[:stretch]
    return c


def stats(v):
    v = np.asarray(v, float)
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def leg(ctx, engine, k, targets, genome, reps, hbm_gbs, expect_hits=None):
    nk_t, nk_g = targets.total_kmers(k), genome.total_kmers(k)
    table = engine.CopyTable(ctx, k, max(1, nk_t), 1)
    distinct = table.insert(targets)
    ins = engine.copies_last_timing()["insert_ms"]
    hits = table.count(0, genome)  # warm
    counts, profiles = [], []
    for _ in range(reps):
        table.clear(0)
        assert table.count(0, genome) == hits
        counts.append(engine.copies_last_timing()["count_ms"])
        hist, valid = table.profile(targets)
        profiles.append(engine.copies_last_timing()["profile_ms"])
    table.close()
    assert (hist.sum(axis=2) == valid[:, None]).all()
    if expect_hits is not None:
        assert hits == expect_hits, (hits, expect_hits)
    engine.synteny_counts(ctx, k, genome, genome)  # warm
    mates = []
    for _ in range(reps):
        engine.synteny_counts(ctx, k, genome, genome)
        mates.append(engine.synteny_last_timing()["mates_ms"])
    cm, mm = float(np.median(counts)), float(np.median(mates))
    slots = 2
    while slots < 2 * max(1, nk_t):
        slots *= 2
    return dict(target_positions=nk_t, distinct_keys=distinct, table_slots=slots, load=round(distinct / slots, 3), genome_positions=nk_g,
                hits=hits, hit_frac=round(hits / max(1, nk_g), 4), insert_ms=round(ins, 4), count_ms=stats(counts), profile_ms=stats(profiles),
                count_g_positions_per_s=round(nk_g / cm / 1e6, 2), profile_g_positions_per_s=round(nk_t / float(np.median(profiles)) / 1e6, 3),
                floor_ms_at_hbm=round(nk_g * 0.375 / hbm_gbs / 1e6, 4), count_over_floor=round(cm / (nk_g * 0.375 / hbm_gbs / 1e6), 1),
                mates_ms=stats(mates), mates_g_positions_per_s=round(nk_g / mm / 1e6, 2), count_over_mates=round(cm / mm, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--contigs", type=int, default=5)
    ap.add_argument("-k", type=int, default=21)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--genes", type=int, default=20)
    ap.add_argument("--gene-len", type=int, default=3000)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the HBM rate the streaming floor is quoted at (GB/s)")
    ap.add_argument("--lib", default=None, help="another build of libpanagram_hip.so to load")
    a = ap.parse_args()
    from panagram_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    from panagram_amd import engine
    import torch
    ctx = engine.Context(0)
    dev = torch.device("cuda", ctx.device)
    gen = torch.Generator(device=dev).manual_seed(a.seed)
    n = int(a.mb * 1e6) // a.contigs
    chroms = [torch.randint(0, 4, (n + 1000 * i,), dtype=torch.uint8, device=dev, generator=gen) for i in range(a.contigs)]
    genome = packed(ctx, engine, chroms)
    out = dict(lib=a.lib or "product", mb=a.mb, contigs=a.contigs, k=a.k, reps=a.reps, hbm_gbs=a.hbm_gbs, bytes_per_position=0.375)
    rng = np.random.default_rng(a.seed)
    at = rng.integers(0, n - a.gene_len, a.genes)
    genes = packed(ctx, engine, [chroms[i % a.contigs][int(s):int(s) + a.gene_len] for i, s in enumerate(at)])
    out["genes"] = leg(ctx, engine, a.k, genes, genome, a.reps, a.hbm_gbs)
    genes.close()
    first = packed(ctx, engine, chroms[:1])
    out["chromosome"] = leg(ctx, engine, a.k, first, first, a.reps, a.hbm_gbs, expect_hits=first.total_kmers(a.k))
    first.close()
    genome.close()
    rep = [with_repeats(c, gen) for c in chroms]
    del chroms
    repeats = packed(ctx, engine, rep)
    units = [b"A", b"AC", b"ACG", b"ACGTC"]
    targets = engine.SeqSet.from_host(ctx, [u * (120 // len(u)) for u in units])
    out["repeats"] = leg(ctx, engine, a.k, targets, repeats, a.reps, a.hbm_gbs)
    targets.close()
    repeats.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
