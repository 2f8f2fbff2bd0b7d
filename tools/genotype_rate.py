"""The allele kernels on genomes of real size: k_allele_insert and k_allele_support, timed with HIP events, beside the three
k_copy_count passes of a `genotype` run and the composition they replace.

    python tools/genotype_rate.py [--mb 100] [--contigs 5] [-k 21] [--div 0.01] [--fastq-gib 1.0] [--read-len 150]

Genome A: --mb megabases in --contigs chromosomes, i.i.d. uniform, drawn with torch on the GPU and packed there; genome B: A with
a substitution at --div of its bases.  The variants are engine.synteny_variants' own (neighbouring substitutions closer than k
come out as one mnp).  The sample: --fastq-gib GiB of four-line FASTQ text, error-free reads of --read-len bases of B from
uniform starts, written on the host and joined on the GPU in batches of 2^28 bytes (SeqSet.from_fastq), as `genotype` streams a
read file.  Reported, in milliseconds: k_allele_insert of A's and of B's ranges, k_copy_count of A, of B and of the reads (the sum
over the batches; the FASTQ kernels' time beside it), k_allele_support of A's and of B's ranges (engine.genotype_last_timing,
engine.copies_last_timing, engine.place_last_timing), the genotypes, and the bytes that cross PCIe for the ranges: 16 per piece
up, 16 per piece down.  Then, on a tenth of the sites, the composition this replaces: SeqSet.slice of one piece per allele (starts
rounded down to 32 bases, as slice wants them), CopyTable.insert of the pieces, the three planes counted again, and
CopyTable.profile(track=True) with its download of a depth per position and plane — host wall-clock times around each call, the
stream synchronised — and its bytes.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

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


def piece_count(ranges, lens, k):
    """the pieces of 64 windows the ranges are cut into (pg_genotype_host.h)"""
    c, s, l = (np.asarray(x).astype(np.int64) for x in ranges)
    L = np.asarray(lens, np.int64)[c]
    w = (np.minimum(L - k + 1, s + l) - np.maximum(0, s - k + 1)).clip(0)
    return int(((w + 63) // 64).sum())


def fastq_batches(genome_ascii, total_bytes, read_len, batch_bytes, seed):
    """FASTQ text of reads cut from the uint8 arrays of ``genome_ascii`` at uniform starts, ``batch_bytes`` at a time"""
    rng = np.random.default_rng(seed)
    rec = 3 + read_len + 3 + read_len + 1
    lens = np.array([len(c) for c in genome_ascii], np.int64)
    left = int(total_bytes) // rec
    while left > 0:
        n = min(left, batch_bytes // rec)
        out = np.empty((n, rec), np.uint8)
        out[:, :3] = np.frombuffer(b"@r\n", np.uint8)
        out[:, 3 + read_len:6 + read_len] = np.frombuffer(b"\n+\n", np.uint8)
        out[:, 6 + read_len:6 + 2 * read_len] = ord("I")
        out[:, -1] = ord("\n")
        which = rng.integers(0, len(genome_ascii), n)
        for c, seq in enumerate(genome_ascii):
            rows = np.flatnonzero(which == c)
            starts = rng.integers(0, lens[c] - read_len, len(rows))
            out[rows, 3:3 + read_len] = seq[starts[:, None] + np.arange(read_len)[None, :]]
        left -= n
        yield out.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--contigs", type=int, default=5)
    ap.add_argument("-k", type=int, default=21)
    ap.add_argument("--div", type=float, default=0.01)
    ap.add_argument("--fastq-gib", type=float, default=1.0)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--batch-bytes", type=int, default=1 << 28)
    ap.add_argument("--min-count", type=int, default=2)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    from panagram_amd import engine, genotype, synteny
    import torch
    k = a.k
    ctx = engine.Context(0)
    dev = torch.device("cuda", ctx.device)
    gen = torch.Generator(device=dev).manual_seed(a.seed)
    n = int(a.mb * 1e6) // a.contigs
    ca = [torch.randint(0, 4, (n + 1000 * i,), dtype=torch.uint8, device=dev, generator=gen) for i in range(a.contigs)]
    cb = []
    for c in ca:
        hit = torch.rand(c.numel(), device=dev, generator=gen) < a.div
        step = torch.randint(1, 4, (c.numel(),), dtype=torch.uint8, device=dev, generator=gen)
        cb.append(torch.where(hit, (c + step) & 3, c))
    ss_a, ss_b = packed(ctx, engine, ca), packed(ctx, engine, cb)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    b_ascii = [acgt[c.cpu().numpy()] for c in cb]
    del ca, cb
    got = engine.synteny_variants(ctx, k, ss_a, ss_b)
    vc, pa, la, pb, lb = (np.asarray(x, np.int64) for x in got[:5])
    cbn, ob = synteny.locate(pb, synteny.contig_offsets([int(x) for x in ss_b.lens]))
    ra = (vc.astype(np.uint32), pa.astype(np.uint64), la.astype(np.uint64))
    rb = (cbn.astype(np.uint32), ob.astype(np.uint64), lb.astype(np.uint64))
    sites = len(vc)
    out = dict(mb=a.mb, contigs=a.contigs, k=k, div=a.div, sites=sites, ref_bases=int(la.sum()), alt_bases=int(lb.sum()),
               variant_classes=dict(zip(synteny.VARIANT_CLASSES, (int(x) for x in got[9]))))
    capacity = int(la.sum() + lb.sum()) + 2 * (k - 1) * sites
    table = engine.CopyTable(ctx, k, capacity, 3)
    ins = []
    for ss, r in ((ss_a, ra), (ss_b, rb)):
        distinct = table.insert_ranges(ss, *r)
        ins.append(dict(ms=round(engine.genotype_last_timing()["insert_ms"], 4), distinct=distinct))
    out["allele_insert"] = dict(a=ins[0], b=ins[1], capacity_keys=capacity)
    counts = {}
    for name, plane, ss in (("a", 0, ss_a), ("b", 1, ss_b)):
        hits = table.count(plane, ss)
        counts[name] = dict(ms=round(engine.copies_last_timing()["count_ms"], 4), hits=hits, positions=ss.total_kmers(k))
    reads = dict(ms=0.0, fastq_ms=0.0, hits=0, reads=0, batches=0, text_bytes=0, host_text_s=0.0)
    first_batch = None
    t0 = time.perf_counter()
    for buf in fastq_batches(b_ascii, a.fastq_gib * (1 << 30), a.read_len, a.batch_bytes, a.seed + 1):
        reads["host_text_s"] += time.perf_counter() - t0
        rs, nreads, used = engine.SeqSet.from_fastq(ctx, buf)
        assert used == len(buf)
        reads["fastq_ms"] += engine.place_last_timing()["fastq_ms"]
        reads["hits"] += table.count(2, rs)
        reads["ms"] += engine.copies_last_timing()["count_ms"]
        reads["reads"] += int(nreads)
        reads["batches"] += 1
        reads["text_bytes"] += len(buf)
        if first_batch is None:
            first_batch = rs
        else:
            rs.close()
        t0 = time.perf_counter()
    for f in ("ms", "fastq_ms", "host_text_s"):
        reads[f] = round(reads[f], 4)
    counts["reads"] = reads
    out["copy_count"] = counts
    sup = []
    for ss, r, own, other in ((ss_a, ra, 0, 1), (ss_b, rb, 1, 0)):
        s = table.allele_support(ss, *r, own, other, 2, a.min_count)
        sup.append(s)
    ms = []
    for ss, r, own, other in ((ss_a, ra, 0, 1), (ss_b, rb, 1, 0)):  # (a second time: the first call's launches were the kernel's first)
        table.allele_support(ss, *r, own, other, 2, a.min_count)
        ms.append(round(engine.genotype_last_timing()["support_ms"], 4))
    pieces = [piece_count(ra, ss_a.lens, k), piece_count(rb, ss_b.lens, k)]
    gt, flag = genotype.call(sup[0][1], sup[0][2], sup[1][1], sup[1][2], 0.5)
    out["allele_support"] = dict(a_ms=ms[0], b_ms=ms[1], windows=int(sup[0][0].sum() + sup[1][0].sum()), inf=int(sup[0][1].sum() + sup[1][1].sum()),
                                 seen=int(sup[0][2].sum() + sup[1][2].sum()), pieces=pieces,
                                 bytes_up=16 * sum(pieces), bytes_down=16 * sum(pieces),
                                 genotypes={g: int((gt == g).sum()) for g in genotype.GENOTYPES},
                                 uninformative=int((flag == "uninformative").sum()))
    table.close()
    # the composition this replaces, on a tenth of the sites
    tenth = slice(0, sites, 10)
    comp = dict(sites=len(vc[tenth]))
    ctx.synchronize()
    t0 = time.perf_counter()
    cut = []
    for ss, (c, s, l) in ((ss_a, ra), (ss_b, rb)):
        c, s, l = c[tenth].astype(np.int64), s[tenth].astype(np.int64), l[tenth].astype(np.int64)
        L = np.asarray(ss.lens, np.int64)[c]
        lo = np.maximum(0, s - k + 1) // 32 * 32
        hi = np.minimum(L, s + l + k - 1)
        cut.append(ss.slice(list(zip(c.tolist(), lo.tolist(), (hi - lo).tolist()))))
    ctx.synchronize()
    comp["slice_s"] = round(time.perf_counter() - t0, 4)
    positions = sum(x.total_kmers(k) for x in cut)
    t2 = engine.CopyTable(ctx, k, max(1, positions), 3)
    t0 = time.perf_counter()
    for x in cut:
        t2.insert(x)
    comp["insert_s"] = round(time.perf_counter() - t0, 4)
    t0 = time.perf_counter()
    t2.count(0, ss_a)
    t2.count(1, ss_b)
    t2.count(2, first_batch)  # (one batch of the reads: the planes' contents do not change what the profile costs)
    comp["count_s"] = round(time.perf_counter() - t0, 4)
    t0 = time.perf_counter()
    down = 0
    for x in cut:
        hist, valid, depths = t2.profile(x, track=True)
        down += depths.nbytes + len(x.lens) * (3 * 64 + 1) * 4  # (the tracks, and one chunk's partials per piece)
    comp["profile_track_s"] = round(time.perf_counter() - t0, 4)
    comp["profile_kernel_ms_last"] = round(engine.copies_last_timing()["profile_ms"], 4)
    comp["positions"] = positions
    comp["bytes_down"] = down
    comp["bytes_down_per_site"] = round(down / max(1, comp["sites"]), 1)
    comp["copied_bases"] = int(sum(int(np.asarray(x.lens, np.int64).sum()) for x in cut))
    out["composition_on_a_tenth"] = comp
    t2.close()
    for x in cut + [first_batch, ss_a, ss_b]:
        x.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
