"""k_bgzf_inflate's output rate on one anchor's bitmap.1.gz, beside 16 host threads of zlib on the same blocks, and the
GPU part of `annotate` (read back + per-gene windows) for a 3 Gb-class anchor with ~40 000 genes.

    python tools/inflate_rate.py [--rows1 3000000000] [--rows8 400000000] [--genes 40000] [--out DIR]

Rows are synthetic bitmaps: runs of equal rows (mean length ~40) drawn from a small palette, one-byte rows (configs[1]
shape, 8 genomes) and 8-byte rows (64 genomes), written by the project's host BGZF writer as Index.run() writes them."""
import argparse
import os
import struct
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from panagram_amd import engine  # noqa: E402


def synth_rows(nrows, nb, rng, chunk=1 << 26):
    pal = rng.integers(0, 256, (48, nb), dtype=np.uint8)
    pal[0] = 0xFF
    done = 0
    while done < nrows:
        n = min(chunk, nrows - done)
        k = n // 20 + 1
        runs = rng.geometric(1 / 40, k)
        ids = rng.choice(len(pal), k, p=np.r_[0.5, np.full(len(pal) - 1, 0.5 / (len(pal) - 1))])
        rows = np.repeat(pal[ids], runs, axis=0)
        while len(rows) < n:
            rows = np.concatenate([rows, rows])
        yield rows[:n]
        done += n


def blocks(path):
    raw = open(path, "rb").read()
    out, off = [], 0
    while off < len(raw):
        bsize = struct.unpack_from("<H", raw, off + 16)[0] + 1
        out.append(raw[off + 18:off + bsize - 8])
        off += bsize
    return out


def host_rate(path, threads=16):
    bl = blocks(path)
    t = time.perf_counter()
    with ThreadPoolExecutor(threads) as pool:
        n = sum(pool.map(lambda b: len(zlib.decompress(b, -15)), bl, chunksize=64))
    return n, time.perf_counter() - t, len(bl)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows1", type=int, default=3_000_000_000)
    ap.add_argument("--rows8", type=int, default=400_000_000)
    ap.add_argument("--genes", type=int, default=40000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    ctx = engine.Context(0)
    d = a.out or tempfile.mkdtemp()
    os.makedirs(d, exist_ok=True)
    for ngen, nrows in ((8, a.rows1), (64, a.rows8)):
        nb = (ngen + 7) // 8
        gz = os.path.join(d, f"bitmap{nb}.1.gz")
        w = engine.BgzfWriter(gz, level=6 | (engine.BgzfWriter.RLE if nb == 1 else engine.BgzfWriter.ROWS(nb)), threads=16)
        for rows in synth_rows(nrows, nb, rng):
            w.write(rows)
        w.close(gz[:-2] + "gzi")
        # 24 chromosomes of equal size
        nk = np.full(24, nrows // 24, np.int64)
        nk[-1] += nrows - nk.sum()
        payload = nrows * nb
        times = []
        for rep in range(3):
            t = time.perf_counter()
            res = engine.AnchorResult.from_bgzf(ctx, 21, ngen, nk, gz, gz[:-2] + "gzi")
            times.append(time.perf_counter() - t)
            if rep < 2:
                res.close()
        n, th, nblk = host_rate(gz)
        assert n == payload
        print(f"{nb}-byte rows ({ngen} genomes): {payload / 1e9:.2f} GB payload, {os.path.getsize(gz) / 1e6:.1f} MB compressed, "
              f"{nblk} BGZF blocks")
        print(f"  GPU read back (file -> pinned -> HBM -> k_bgzf_inflate -> rows), wall: "
              + ", ".join(f"{t:.3f} s" for t in times) + f"  = {payload / min(times) / 1e9:.1f} GB/s of output (best)")
        print(f"  host, 16 threads of zlib on the same blocks (from memory): {th:.3f} s = {payload / th / 1e9:.1f} GB/s")
        if nb == 1:  # the GPU part of annotate: per-gene windows over every chromosome
            per = a.genes // 24
            t = time.perf_counter()
            for ci in range(24):
                st = np.sort(rng.integers(0, nk[ci] - 100000, per)).astype(np.uint64)
                en = st + rng.integers(1000, 60000, per).astype(np.uint64)
                res.window_stats(ci, st, en, step=1, colsums=False)
            tw = time.perf_counter() - t
            print(f"  annotate, {per * 24} genes on 24 chromosomes: read back {min(times):.3f} s + window_stats {tw:.3f} s")
        res.close()
    ctx.close()


if __name__ == "__main__":
    main()
