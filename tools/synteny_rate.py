"""The synteny kernels on genomes of real size: k_pos_insert (both sides), k_pos_mates and k_mate_runs, timed with HIP events.

    python tools/synteny_rate.py [--mb 100] [--contigs 5] [-d 0.01] [-k 21] [--reps 5]

Two synthetic genomes of --mb megabases in --contigs chromosomes: A i.i.d. uniform, B = A with substitutions at rate d, one
chromosome inverted as a whole and two exchanged, so both strands and a translocation are in the run.  The sequences are drawn
with torch on the GPU and packed there (SeqSet.load_dev).  engine.synteny_segments runs once warm (the code object's load, the
first allocations) and --reps times; each kernel's time is the HIP-event interval around its launch that the library records
(engine.synteny_last_timing), the median over the repetitions with the spread beside it.  The call time is a host clock around the
synchronous call (table allocation and memset, job lists, both launches of k_mate_runs, the read-back of the runs).
Rates: k-mer positions per second of the side a kernel walks; for k_mate_runs the bytes of the mates array it reads (once per
launch) per second.  Checked at this size: the mated positions equal the sum of the runs' lengths, the runs are sorted, and
with d = 0 every chromosome is one run.  Prints one JSON line.

--blocks adds the blocks (pg_blocks.hip) on the same genomes: engine.synteny_blocks with --min-run / --max-gap / --max-shift, the
seven kernel times (engine.synteny_blocks_last_timing), the call's wall time, and beside it the wall time of the route without
k_run_blocks to the same answer: engine.synteny_segments emitting and downloading every run, then the chain built on the host
with numpy (chain_host below: the link rule on whole arrays, the blocks by np.add.reduceat).  The two answers must be equal.

--variants adds the variants (pg_variants.hip) on the same genomes and with the same three parameters: engine.synteny_variants,
the nine kernel times (engine.synteny_variants_last_timing: the seven above, then k_link_variants counting and emitting), the call's
wall time, the links of every class, and two checks against the blocks of the same parameters: the links are the sum of (runs - 1)
over the blocks, and on this workload, which has substitutions only, every variant is a snp or an mnp."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from panagram_amd import engine  # noqa: E402


def genomes(ctx, mb, ncontigs, d, seed):
    """(SeqSet A, SeqSet B): B's chromosome 0 is A's reverse-complemented, B's last two are A's exchanged"""
    import torch
    dev = torch.device("cuda", ctx.device)
    gen = torch.Generator(device=dev).manual_seed(seed)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    n = int(mb * 1e6) // ncontigs
    lens = [n + 1000 * i for i in range(ncontigs)]
    a = [torch.randint(0, 4, (m,), dtype=torch.uint8, device=dev, generator=gen) for m in lens]
    b = []
    for c in a:
        mut = torch.rand(c.shape, device=dev, generator=gen) < d
        shift = torch.randint(1, 4, c.shape, dtype=torch.uint8, device=dev, generator=gen)
        b.append(torch.where(mut, (c + shift) & 3, c))
    b[0] = 3 - torch.flip(b[0], [0])
    if ncontigs >= 3:
        b[-1], b[-2] = b[-2], b[-1]
    sets = []
    for contigs in (a, b):
        ss = engine.SeqSet(ctx, [int(c.numel()) for c in contigs])
        for i, c in enumerate(contigs):
            t = acgt[c.long()]
            torch.cuda.synchronize()
            ss.load_dev(i, t.data_ptr(), int(t.numel()))
            ctx.synchronize()
        sets.append(ss)
    return sets


def chain_host(rc, rs, re_, rm, lens_b, min_run, max_gap, max_shift):
    """the blocks of include/panagram_hip.h from run arrays on the host, vectorised: [n, 8] int64"""
    rc, rs, re_, rm = (np.asarray(x, np.int64) for x in (rc, rs, re_, rm))
    n = re_ - rs
    keep = n >= min_run
    rc, rs, re_, rm, n = rc[keep], rs[keep], re_[keep], rm[keep], n[keep]
    if not len(rc):
        return np.zeros((0, 8), np.int64)
    strand = rm & 1
    ml = np.where(strand == 1, rm - 2 * (n - 1), rm + 2 * (n - 1))
    d_a = rs[1:] - (re_[:-1] - 1)
    d_b = np.where(strand[1:] == 1, (ml[:-1] >> 1) - (rm[1:] >> 1), (rm[1:] >> 1) - (ml[:-1] >> 1))
    edges = np.cumsum(np.asarray(lens_b, np.int64))
    same_b = np.searchsorted(edges, ml[:-1] >> 1, side="right") == np.searchsorted(edges, rm[1:] >> 1, side="right")
    link = ((rc[1:] == rc[:-1]) & (strand[1:] == strand[:-1]) & (d_a >= 1) & (d_a <= max_gap) & (d_b >= 1) & (d_b <= max_gap) &
            (np.abs(d_a - d_b) <= max_shift) & same_b)
    first = np.flatnonzero(np.concatenate([[True], ~link]))
    last = np.concatenate([first[1:], [len(rc)]]) - 1
    shifted = np.concatenate([[0], link & (d_a != d_b)]).astype(np.int64)
    return np.stack([rc[first], rs[first], re_[last], rm[first], ml[last], np.add.reduceat(n, first), last - first + 1,
                     np.add.reduceat(shifted, first)], axis=1)


def blocks_leg(ctx, a, ssa, ssb, out):
    params = dict(min_run=a.min_run, max_gap=a.max_gap, max_shift=a.max_shift)
    blk = engine.synteny_blocks(ctx, a.k, ssa, ssb, **params)  # warm
    cap = len(blk[0])
    nruns = blk[10]
    times, calls, host = [], [], []
    lens_b = [int(n) for n in ssb.lens]
    for _ in range(a.reps):  # (the two routes in turn)
        t0 = time.perf_counter()
        got = engine.synteny_blocks(ctx, a.k, ssa, ssb, cap=cap, **params)
        calls.append(time.perf_counter() - t0)
        times.append(engine.synteny_blocks_last_timing())
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got[:8], blk[:8]))  # the same on every call
        t0 = time.perf_counter()
        rc, rs, re_, rm, _, _ = engine.synteny_segments(ctx, a.k, ssa, ssb, cap=nruns)
        t1 = time.perf_counter()
        want = chain_host(rc, rs, re_, rm, lens_b, **params)
        host.append((time.perf_counter() - t0, t1 - t0))
    have = np.stack(blk[:8], axis=1).astype(np.int64)
    res = dict(params, blocks=len(have), runs=nruns, runs_per_block=round(nruns / max(1, len(have)), 1),
               shifted_links=int(have[:, 7].sum()), equal_to_host_chain=bool(have.shape == want.shape and (have == want).all()),
               bytes_down=dict(blocks=int(have.shape[0]) * 32, runs=int(nruns) * 12))
    for name in times[0]:
        v = np.array([t[name] for t in times])
        res[name] = dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))
    for name in ("blocks_count_ms", "blocks_emit_ms"):
        med = res[name]["median"]
        res[name]["runs_gb_per_s"] = round(nruns * 12 / med / 1e6, 1) if med > 0 else None
    res["call_s"] = dict(median=round(float(np.median(calls)), 4), min=round(min(calls), 4), max=round(max(calls), 4))
    tot, seg = np.array([h[0] for h in host]), np.array([h[1] for h in host])
    res["host_route_s"] = dict(median=round(float(np.median(tot)), 4), min=round(float(tot.min()), 4), max=round(float(tot.max()), 4),
                               segments_call_median=round(float(np.median(seg)), 4),
                               numpy_chain_median=round(float(np.median(tot - seg)), 4))
    res["gpu_route_faster"] = bool(np.median(calls) < np.median(tot))
    out["blocks"] = res


def variants_leg(ctx, a, ssa, ssb, out):
    params = dict(min_run=a.min_run, max_gap=a.max_gap, max_shift=a.max_shift)
    var = engine.synteny_variants(ctx, a.k, ssa, ssb, **params)  # warm
    cap = len(var[0])
    blk = engine.synteny_blocks(ctx, a.k, ssa, ssb, **params)
    times, calls = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        got = engine.synteny_variants(ctx, a.k, ssa, ssb, cap=cap, **params)
        calls.append(time.perf_counter() - t0)
        times.append(engine.synteny_variants_last_timing())
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got[:10], var[:10]))  # the same on every call
    classes = [int(x) for x in var[9]]
    nruns = var[12]
    res = dict(params, variants=cap, links=var[10], classes=dict(zip(engine.VARIANT_CLASSES, classes)), runs=nruns, blocks=var[13],
               bases_a=int(var[2].astype(np.int64).sum()), bases_b=int(var[4].astype(np.int64).sum()),
               n_flagged=int(((var[5] >> 6) & 1).sum()), bytes_down=cap * 44,
               checks=dict(links_are_block_runs_less_one=bool(var[10] == int((blk[6].astype(np.int64) - 1).sum())),
                           classes_add_up=bool(sum(classes) == var[10] and sum(classes[1:]) == cap),
                           sorted=bool((np.diff(var[0].astype(np.int64) * (1 << 32) + var[1]) > 0).all()),
                           substitutions_only=bool(classes[3] == classes[4] == classes[5] == 0)))
    for name in times[0]:
        v = np.array([t[name] for t in times])
        res[name] = dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))
    for name in ("blocks_count_ms", "variants_count_ms", "variants_emit_ms"):
        med = res[name]["median"]
        res[name]["runs_gb_per_s"] = round(nruns * 12 / med / 1e6, 1) if med > 0 else None
    res["call_s"] = dict(median=round(float(np.median(calls)), 4), min=round(min(calls), 4), max=round(max(calls), 4))
    out["variants"] = res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--contigs", type=int, default=5)
    ap.add_argument("-d", type=float, default=0.01)
    ap.add_argument("-k", type=int, default=21)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--blocks", action="store_true", help="also time engine.synteny_blocks against the host's chain of the runs")
    ap.add_argument("--variants", action="store_true", help="also time engine.synteny_variants: the nine kernel times, the links by class")
    ap.add_argument("--min-run", type=int, default=1)
    ap.add_argument("--max-gap", type=int, default=1000)
    ap.add_argument("--max-shift", type=int, default=100)
    a = ap.parse_args()
    ctx = engine.Context(0)
    ssa, ssb = genomes(ctx, a.mb, a.contigs, a.d, a.seed)
    nka, nkb = ssa.total_kmers(a.k), ssb.total_kmers(a.k)
    slots = 2
    while slots < 2 * (nka + nkb):
        slots *= 2
    out = dict(mb=a.mb, contigs=a.contigs, d=a.d, k=a.k, reps=a.reps, kmers_a=nka, kmers_b=nkb, table_slots=slots,
               table_gb=round(slots * 16 / 1e9, 3), load=round((nka + nkb) / slots, 3))
    runs = engine.synteny_segments(ctx, a.k, ssa, ssb)  # warm
    cap = len(runs[0])
    times, calls = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        got = engine.synteny_segments(ctx, a.k, ssa, ssb, cap=cap)
        calls.append(time.perf_counter() - t0)
        times.append(engine.synteny_last_timing())
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got[:4], runs[:4]))  # the same on every call
    rc, rs, re_, rm, per, nmated = runs
    out.update(runs=len(rc), mated=nmated, mated_frac=round(nmated / max(1, nka), 4), minus_runs=int((rm & 1).sum()),
               checks=dict(mated_is_sum_of_runs=bool(int((re_.astype(np.int64) - rs).sum()) == nmated),
                           sorted=bool((np.diff(rc.astype(np.int64) * (1 << 32) + rs) > 0).all()),
                           one_run_per_contig_at_d0=(bool(len(rc) == a.contigs) if a.d == 0 else None)))
    side = dict(insert_a_ms=nka, insert_b_ms=nkb, mates_ms=nka, runs_count_ms=nka, runs_emit_ms=nka)
    for name, n in side.items():
        v = np.array([t[name] for t in times])
        med = float(np.median(v))
        out[name] = dict(median=round(med, 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4),
                         g_positions_per_s=round(n / med / 1e6, 2) if med > 0 else None)
    for name in ("runs_count_ms", "runs_emit_ms"):
        med = out[name]["median"]
        out[name]["mates_gb_per_s"] = round(nka * 4 / med / 1e6, 1) if med > 0 else None
    out["call_s"] = dict(median=round(float(np.median(calls)), 4), min=round(min(calls), 4), max=round(max(calls), 4))
    if a.blocks:
        blocks_leg(ctx, a, ssa, ssb, out)
    if a.variants:
        variants_leg(ctx, a, ssa, ssb, out)
    ssa.close()
    ssb.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
