"""The locate kernels on genomes of real size: k_hit_runs (count, emit) and k_run_blocks (count, emit), timed with HIP events.

    python tools/locate_rate.py [--mb 100] [--contigs 5] [-k 21] [--reps 5] [--lib PATH]

Two synthetic genomes of --mb megabases in --contigs chromosomes, i.i.d. uniform, drawn with torch on the GPU and packed there
(SeqSet.load_dev), each streamed through a query table of its own:
  genes   --genes pieces of --gene-len bases cut from the first genome: a table the size of a genome's genes, a few percent of
          the windows hit
  few     --few pieces of --few-len bases cut from the second genome: a table of a few sequences, almost no window hits
Per leg the four times of engine.locate_last_timing (the median of --reps calls of PosTable.locate after a warm one, the spread
beside it), the positions per second of k_hit_runs' count pass, and as a yardstick the other route to the same runs on a side of
the same size — k_pos_mates, which writes a mate word per position, then k_mate_runs, which reads them back
(engine.synteny_last_timing of the genome against itself, counting only) — with the streaming floor at --hbm-gbs beside both: the
packed genome is 0.375 byte per position (2 bits of sequence, 1 bit of mask), read once per pass.
Checked at this size: the pieces are found whole — hits at least the pieces' unique k-mers, a locus of all its k-mers for every
piece but the few that share a k-mer with another by chance.
Reported, not gated: there is no threshold for any of it (profiles/locate_rate.txt).  Prints one JSON line."""
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


def stats(v):
    v = np.asarray(v, float)
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def leg(ctx, engine, k, queries, genome, reps, hbm_gbs, pieces, piece_len):
    nk_q, nk_g = queries.total_kmers(k), genome.total_kmers(k)
    table = engine.PosTable(ctx, k, max(1, nk_q))
    table.insert(1, queries)
    unique = int(table.hit_runs(queries)[5].sum())
    got = table.locate(genome, queries)  # warm
    times = {name: [] for name in engine.locate_last_timing()}
    for _ in range(reps):
        again = table.locate(genome, queries)
        assert again[9:] == got[9:] and len(again[0]) == len(got[0])
        for name, ms in engine.locate_last_timing().items():
            times[name].append(ms)
    table.close()
    nhits, nruns, nloci = got[9], got[10], len(got[0])
    whole = int((got[5] == piece_len - k + 1).sum())  # the loci that hold a whole piece
    # (a k-mer that two pieces share by chance repeats among the queries, and takes a position from each)
    assert nhits >= unique and nloci >= pieces and whole >= pieces - 16, (nhits, unique, nloci, whole, pieces)
    engine.synteny_counts(ctx, k, genome, genome)  # warm
    mates, runs = [], []
    for _ in range(reps):
        engine.synteny_counts(ctx, k, genome, genome)
        t = engine.synteny_last_timing()
        mates.append(t["mates_ms"])
        runs.append(t["runs_count_ms"])
    count = float(np.median(times["hits_count_ms"]))
    floor = nk_g * 0.375 / hbm_gbs / 1e6
    return dict(query_positions=nk_q, unique_query_positions=unique, genome_positions=nk_g, hits=nhits, hit_frac=round(nhits / max(1, nk_g), 5),
                runs=nruns, loci=nloci, whole_pieces=whole, **{name: stats(v) for name, v in times.items()},
                hits_count_g_positions_per_s=round(nk_g / count / 1e6, 2), floor_ms_at_hbm=round(floor, 4),
                hits_count_over_floor=round(count / floor, 1), mates_ms=stats(mates), mate_runs_count_ms=stats(runs),
                mates_plus_runs_ms=round(float(np.median(mates)) + float(np.median(runs)), 4),
                hits_both_passes_ms=round(count + float(np.median(times["hits_emit_ms"])), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--contigs", type=int, default=5)
    ap.add_argument("-k", type=int, default=21)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--genes", type=int, default=2000)
    ap.add_argument("--gene-len", type=int, default=3000)
    ap.add_argument("--few", type=int, default=5)
    ap.add_argument("--few-len", type=int, default=20000)
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
    out = dict(lib=a.lib or "product", mb=a.mb, contigs=a.contigs, k=a.k, reps=a.reps, hbm_gbs=a.hbm_gbs, bytes_per_position=0.375)
    n = int(a.mb * 1e6) // a.contigs
    for name, seed, pieces, piece_len in (("genes", a.seed, a.genes, a.gene_len), ("few", a.seed + 1, a.few, a.few_len)):
        gen = torch.Generator(device=dev).manual_seed(seed)
        chroms = [torch.randint(0, 4, (n + 1000 * i,), dtype=torch.uint8, device=dev, generator=gen) for i in range(a.contigs)]
        genome = packed(ctx, engine, chroms)
        # piece i: chromosome i % contigs, a slot of its own there (the pieces do not overlap), a random place inside the slot
        slots = -(-pieces // a.contigs)
        room = (n - piece_len) // slots
        assert room >= piece_len, "the pieces do not fit the chromosomes"
        jitter = np.random.default_rng(seed).integers(0, room - piece_len + 1, pieces)
        at = [(i // a.contigs) * room + int(jitter[i]) for i in range(pieces)]
        queries = packed(ctx, engine, [chroms[i % a.contigs][s:s + piece_len] for i, s in enumerate(at)])
        del chroms
        out[name] = leg(ctx, engine, a.k, queries, genome, a.reps, a.hbm_gbs, pieces, piece_len)
        queries.close()
        genome.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
