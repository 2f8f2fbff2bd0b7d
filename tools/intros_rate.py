"""`intros`'s binning step on an index of real size: the wall time of a whole Genome.kmer_similarity_bins call at --stp 1
and --stp 100 (the file read, the inflate into HBM, k_bin_colsums and the frames; host clock around the synchronous
call), beside the reference's host path at --stp 100 (bitmap rows read on the host, one pandas frame per
chromosome, groupby sums: call_introgressions.py's bitmap_to_bins).

    python tools/intros_rate.py [--genomes 16] [--chroms 4] [--mb 40] [--dir DIR] [--only-gpu]

The index: ``--genomes`` synthetic genomes (base + 1 % substitutions) of ``--chroms`` chromosomes of ``--mb`` Mb, one anchor,
built by Index.run(); its bitmap.1 rows (genomes / 8 bytes each) exceed the 256 MiB Infinity Cache.  It is kept in ``--dir``
and reused by a later run (``--only-gpu``: just the two GPU calls, once each — the run to put under
``rocprofv3 --kernel-trace --stats`` for k_bin_colsums' and k_bgzf_inflate's own times)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from panagram_amd import index as pidx  # noqa: E402

ACGT = np.frombuffer(b"ACGT", np.uint8)


def write_fasta(path, chroms, seqs, width=80):
    with open(path, "wb") as f:
        for nm, s in zip(chroms, seqs):
            f.write(b">" + nm.encode() + b"\n")
            full = len(s) // width * width
            body = np.concatenate([ACGT[s[:full]].reshape(-1, width), np.full((full // width, 1), 10, np.uint8)], axis=1)
            f.write(body.tobytes())
            if full < len(s):
                f.write(ACGT[s[full:]].tobytes() + b"\n")


def build_index(d, n, nchr, mb, seed=5):
    rng = np.random.default_rng(seed)
    chroms = [f"chr{i + 1}" for i in range(nchr)]
    base = [rng.integers(0, 4, int(mb * 1e6), dtype=np.uint8) for _ in chroms]
    rows = ["name\tfasta"]
    for g in range(n):
        seqs = base if g == 0 else [np.where(rng.random(len(b)) < 0.01, (b + rng.integers(1, 4, len(b), dtype=np.uint8)) & 3, b)
                                    .astype(np.uint8) for b in base]
        fa = os.path.join(d, f"g{g}.fa")
        write_fasta(fa, chroms, seqs)
        rows.append(f"g{g}\t{fa}")
    with open(os.path.join(d, "samples.tsv"), "w") as f:
        f.write("\n".join(rows) + "\n")
    t0 = time.perf_counter()
    pidx.Index(os.path.join(d, "samples.tsv"), prefix=os.path.join(d, "idx"), k=21, anchor_genomes=["g0"]).run()
    for g in range(n):
        os.remove(os.path.join(d, f"g{g}.fa"))
    return time.perf_counter() - t0


def host_bins(g, step, bin_size):
    """the reference's path: genome.query rows on the host, then bitmap_to_bins' pandas groupby"""
    out = {}
    for c in g.chrs.index:
        q = g.query(c, 0, int(g.chrs.loc[c, "size"]), step)
        b = q.set_index(q.index // bin_size)
        sums = b.groupby(level=0).sum()
        sums = sums.set_index(sums.index * bin_size).T
        out[c] = sums.div(sums.max(axis=0), axis=1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=16)
    ap.add_argument("--chroms", type=int, default=4)
    ap.add_argument("--mb", type=float, default=40)
    ap.add_argument("--bin", type=int, default=1_000_000)
    ap.add_argument("--dir", default=os.path.join(tempfile.gettempdir(), "intros_rate"))
    ap.add_argument("--only-gpu", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    res = dict(genomes=a.genomes, chroms=a.chroms, mb=a.mb, bin=a.bin)
    if not os.path.exists(os.path.join(a.dir, "idx", "config.yaml")):
        res["index_build_s"] = round(build_index(a.dir, a.genomes, a.chroms, a.mb), 2)
    idx = pidx.Index(os.path.join(a.dir, "idx"), mode="r")
    g = idx["g0"]
    g.load_chrs()
    nrows = int(g.chrs["size"].sum())
    res["rows1"] = nrows
    res["row_bytes"] = g.nbytes
    res["rows1_mib"] = round(nrows * g.nbytes / 2 ** 20, 1)
    res["bitmap1_gz_mib"] = round(os.path.getsize(g.bitmap_gz_fname(1)) / 2 ** 20, 1)
    reps = 1 if a.only_gpu else 3
    for step in (1, 100):
        g.kmer_similarity_bins(step=step, bin_size=a.bin)  # (first call: code objects, context)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fr = g.kmer_similarity_bins(step=step, bin_size=a.bin)
            ts.append(time.perf_counter() - t0)
        res[f"call_wall_stp{step}_s"] = round(min(ts), 4)
        res[f"gpu_stp{step}_bins"] = int(sum(f.shape[1] for f in fr.values()))
    if not a.only_gpu:
        g.init_read()
        t0 = time.perf_counter()
        hb = host_bins(g, 100, a.bin)
        res["host_pandas_stp100_s"] = round(time.perf_counter() - t0, 3)
        gb = g.kmer_similarity_bins(step=100, bin_size=a.bin)
        res["host_equals_gpu_stp100"] = all(np.allclose(hb[c].to_numpy(float), gb[c].to_numpy(float), equal_nan=True)
                                            for c in gb)
        res["host_stp100_over_call_stp1"] = round(res["host_pandas_stp100_s"] / res["call_wall_stp1_s"], 2)
    idx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
