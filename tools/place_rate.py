"""The kernels of `place` on inputs of real size, timed with HIP events and with the wall clock.

    python tools/place_rate.py [--mb 100] [--contigs 5] [-k 21] [--genomes 8,64] [--fastq-mb 1024] [--e2e-mb 0] [--reps 5]

agree   an anchor of --mb megabases in --contigs chromosomes, i.i.d. uniform, drawn with torch on the GPU and packed there; a count
        table of its k-mers with the anchor itself counted into plane 0 (every valid row is held at min_count 1); a rows container of
        N genomes (each of --genomes) filled with random bytes.  k_sample_agree over bins of 100 000 rows
        (engine.place_last_timing) against the two passes that do the same lookups and the same row reads apart: k_copy_profile of
        the anchor (one plane, no track: engine.copies_last_timing) and k_bin_colsums over the same bins (no event timing in the
        library: the call's wall time, beside the wall time of the other two calls).  Medians of --reps calls after a warm one.
fastq   a synthetic four-line FASTQ of --fastq-mb MiB (tools/make_fastq.py: 150-base reads), in memory and in a file:
        SeqSet.from_fastq — the kernels' HIP-event time and the whole call, upload included — against index.read_fastq_joined of the
        file plus SeqSet.from_host of what it returns.  Checked: both give the same contig length.
e2e     --e2e-mb M > 0: eight genomes of M megabases (an anchor and seven copies with 1 % substitutions), indexed in a temporary
        directory, and 30-fold 150-base reads of the second one: the seconds of Index.place (bin size 100 000, min_count 2).
Prints one JSON line."""
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


def med(v):
    v = np.asarray(v, float)
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def device_bytes(ptr, nbytes, device):
    import torch

    class _Wrap:
        __cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 3}
    return torch.as_tensor(_Wrap(), device=torch.device("cuda", device))


def agree_leg(ctx, engine, a, ngenomes):
    import torch
    from copies_rate import packed
    dev = torch.device("cuda", ctx.device)
    gen = torch.Generator(device=dev).manual_seed(a.seed)
    n = int(a.mb * 1e6) // a.contigs
    chroms = [torch.randint(0, 4, (n + 1000 * i,), dtype=torch.uint8, device=dev, generator=gen) for i in range(a.contigs)]
    anchor = packed(ctx, engine, chroms)
    del chroms
    k = a.k
    nk = [int(x) - k + 1 for x in anchor.lens]
    table = engine.CopyTable(ctx, k, sum(nk), 1)
    table.insert(anchor)
    hits = table.count(0, anchor)
    shell = engine.SeqSet(ctx, [int(x) for x in anchor.lens])
    res = engine.AnchorResult.rows_container(ctx, k, ngenomes, shell, colsums=False)
    (ptr, size), _ = res.device_ptrs()
    buf = device_bytes(ptr, size, ctx.device)
    for s in range(0, size, 1 << 28):
        e = min(size, s + (1 << 28))
        buf[s:e] = torch.randint(0, 256, (e - s,), dtype=torch.uint8, device=dev, generator=gen)
    torch.cuda.synchronize()
    res.rows_epilogue()
    ci = np.concatenate([np.full(-(-m // a.bin_size), i, np.uint32) for i, m in enumerate(nk)])
    st = np.concatenate([np.arange(0, m, a.bin_size, dtype=np.uint64) for m in nk])
    en = np.concatenate([np.minimum(np.arange(0, m, a.bin_size, dtype=np.uint64) + np.uint64(a.bin_size), np.uint64(m)) for m in nk])
    agree_ms, agree_wall, prof_ms, prof_wall, bins_wall = [], [], [], [], []
    for r in range(a.reps + 1):
        t0 = time.perf_counter()
        valid, held, col, both = table.sample_agree(0, 1, anchor, res, ci, st, en)
        t1 = time.perf_counter()
        hist, v = table.profile(anchor)
        t2 = time.perf_counter()
        cs, kept = res.bin_colsums(ci, st, en)
        t3 = time.perf_counter()
        if r:
            agree_ms.append(engine.place_last_timing()["agree_ms"])
            prof_ms.append(engine.copies_last_timing()["profile_ms"])
            agree_wall.append((t1 - t0) * 1e3)
            prof_wall.append((t2 - t1) * 1e3)
            bins_wall.append((t3 - t2) * 1e3)
    assert int(valid.sum()) == int(v.sum()) == int(held.sum()) == sum(nk) and hits >= sum(nk)
    assert np.array_equal(col, cs) and np.array_equal(col, both)  # (every row valid and held: the fused counts are the column sums)
    for x in (res, shell, table, anchor):
        x.close()
    return dict(genomes=ngenomes, positions=sum(nk), bins=len(ci), row_bytes=(ngenomes + 7) // 8, agree_ms=med(agree_ms),
                agree_g_positions_per_s=round(sum(nk) / float(np.median(agree_ms)) / 1e6, 2), agree_call_wall_ms=med(agree_wall),
                copy_profile_ms=med(prof_ms), copy_profile_call_wall_ms=med(prof_wall), bin_colsums_call_wall_ms=med(bins_wall))


def fastq_leg(ctx, engine, a, tmp):
    from make_fastq import fastq_records, record_bytes
    from panagram_amd import index as pidx
    nrec = max(1, int(a.fastq_mb * (1 << 20)) // record_bytes(150))
    text = fastq_records(nrec, 150, a.seed).reshape(-1)
    path = os.path.join(tmp, "reads.fq")
    text.tofile(path)
    kern, wall = [], []
    for r in range(a.reps + 1):
        t0 = time.perf_counter()
        ss, n, used = engine.SeqSet.from_fastq(ctx, text)
        t1 = time.perf_counter()
        length = int(ss.lens[0])
        ss.close()
        assert n == nrec and used == len(text)
        if r:
            kern.append(engine.place_last_timing()["fastq_ms"])
            wall.append((t1 - t0) * 1e3)
    t0 = time.perf_counter()
    joined = pidx.read_fastq_joined(path)
    t1 = time.perf_counter()
    hs = engine.SeqSet.from_host(ctx, [joined])
    t2 = time.perf_counter()
    assert int(hs.lens[0]) == length == nrec * 151 - 1
    hs.close()
    os.remove(path)
    gb = len(text) / 1e9
    return dict(text_bytes=int(len(text)), records=nrec, kernels_ms=med(kern), kernels_gb_per_s=round(gb / float(np.median(kern)) * 1e3, 2),
                call_wall_ms=med(wall), call_gb_per_s=round(gb / float(np.median(wall)) * 1e3, 2),
                read_fastq_joined_ms=round((t1 - t0) * 1e3, 1), from_host_ms=round((t2 - t1) * 1e3, 1),
                host_path_gb_per_s=round(gb / (t2 - t0), 3))


def e2e_leg(a, tmp):
    from make_fastq import fastq_records
    from panagram_amd import index as pidx
    rng = np.random.default_rng(a.seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    n = int(a.e2e_mb * 1e6) // 2
    base = [rng.integers(0, 4, n, dtype=np.uint8), rng.integers(0, 4, n, dtype=np.uint8)]
    lines = ["name\tfasta\tgff"]
    second = None
    for g in range(8):
        fa = os.path.join(tmp, f"g{g}.fa")
        with open(fa, "wb") as f:
            contigs = []
            for c, codes in enumerate(base):
                if g:
                    codes = codes.copy()
                    hit = np.flatnonzero(rng.random(n) < 0.01)
                    codes[hit] = (codes[hit] + rng.integers(1, 4, len(hit), dtype=np.uint8)) % 4
                contigs.append(codes)
                body = acgt[codes[:n - n % 80]].reshape(-1, 80)
                f.write(b">chr%d\n" % (c + 1))
                f.write(np.concatenate([body, np.full((len(body), 1), 10, np.uint8)], axis=1).tobytes())
                if n % 80:
                    f.write(acgt[codes[n - n % 80:]].tobytes() + b"\n")
            if g == 1:
                second = contigs
        lines.append(f"g{g}\t{fa}\t")
    open(os.path.join(tmp, "samples.tsv"), "w").write("\n".join(lines) + "\n")
    out = os.path.join(tmp, "idx")
    t0 = time.perf_counter()
    pidx.Index(os.path.join(tmp, "samples.tsv"), prefix=out, k=a.k, anchor_genomes=["g0"], lowres_step=100).run()
    t_index = time.perf_counter() - t0
    nreads = 30 * 2 * n // 150
    fq = os.path.join(tmp, "sample.fq")
    with open(fq, "wb") as f:
        for r0 in range(0, nreads, 1 << 20):
            m = min(1 << 20, nreads - r0)
            c = second[(r0 >> 20) & 1]
            at = rng.integers(0, n - 150, m)
            f.write(fastq_records(m, 150, a.seed, seqs=acgt[c[at[:, None] + np.arange(150)[None, :]]]).tobytes())
    idx = pidx.Index(out, mode="r")
    try:
        t0 = time.perf_counter()
        main_, _, summary, stats = idx.place("g0", [fq], bin_size=100000, min_count=2)
        t_place = time.perf_counter() - t0
    finally:
        idx.close()
    called = main_["best"].value_counts().to_dict()
    return dict(genomes=8, mb_per_genome=a.e2e_mb, reads=int(stats["reads"]), read_bases=int(stats["read_bases"]), fastq_bytes=os.path.getsize(fq),
                index_seconds=round(t_index, 2), place_seconds=round(t_place, 2), bins=len(main_), best=called, depth_mode=int(stats["depth_mode"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--contigs", type=int, default=5)
    ap.add_argument("-k", type=int, default=21)
    ap.add_argument("--genomes", default="8,64")
    ap.add_argument("--bin-size", type=int, default=100000)
    ap.add_argument("--fastq-mb", type=float, default=1024.0)
    ap.add_argument("--e2e-mb", type=float, default=0.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    from panagram_amd import engine
    out = dict(mb=a.mb, contigs=a.contigs, k=a.k, bin_size=a.bin_size, reps=a.reps)
    with tempfile.TemporaryDirectory() as tmp:
        ctx = engine.Context(0)
        if a.mb > 0:
            out["agree"] = [agree_leg(ctx, engine, a, int(g)) for g in a.genomes.split(",") if g]
        if a.fastq_mb > 0:
            out["fastq"] = fastq_leg(ctx, engine, a, tmp)
        ctx.close()
        if a.e2e_mb > 0:
            out["e2e"] = e2e_leg(a, tmp)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
