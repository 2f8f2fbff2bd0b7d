"""k_knn_rows at the sizes the UMAP files need, and the host layout behind it.

    python tools/knn_rate.py [--n 30000 300000] [--cols 8 64 128] [--k 4] [--segments 24 1350] [--layout 30000]

Per shape: a random n x N float32 matrix of values c / 8 (what binned pair counts look like), ``engine.knn_rows`` timed by the
host clock around the synchronous call — staging of X, launch and read-back included; best of 3 after a warm call — once as
one segment and once as ``--segments S R``: S segments of R rows.  Printed per run: seconds, pair evaluations per second
(n^2, or S R^2), and the two candidate limits as fractions of the device's peak at 2.4 GHz — vector issue (3 instructions
per value and pair on 256 CUs x 4 SIMDs x 32 lanes) and the LDS array (one 16-byte broadcast read per wave, 4 values and
4 LDS cycles, 256 CUs) — the larger one binds.  ``--layout n``: host seconds of fuzzy_graph and layout (200 epochs beyond 10 000
rows) for n rows at N = 8.  Prints one JSON line at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from panagram_amd import engine, umap  # noqa: E402

LANES_PER_S = 256 * 4 * 32 * 2.4e9
LDS_CYCLES_PER_S = 256 * 2.4e9


def best(f, reps=3):
    f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return min(t)


def report(tag, secs, pairs, cols):
    dt = 8 if cols <= 8 else 32 if cols <= 32 else 64 if cols <= 64 else 128 if cols <= 128 else 32 * -(-cols // 32)
    row = dict(shape=tag, seconds=round(secs, 5), pairs_per_s=pairs / secs, issue_fraction=pairs * dt * 3 / secs / LANES_PER_S,
               lds_fraction=pairs * dt / 4 / 64 * 4 / secs / LDS_CYCLES_PER_S)
    print(f"{tag:34s} {secs * 1e3:10.2f} ms  {row['pairs_per_s']:.3e} pairs/s  issue {row['issue_fraction']:.2f}  "
          f"lds {row['lds_fraction']:.2f}", flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[30000, 300000])
    ap.add_argument("--cols", type=int, nargs="*", default=[8, 64, 128])
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--segments", type=int, nargs=2, default=[24, 1350])
    ap.add_argument("--layout", type=int, default=30000)
    a = ap.parse_args()
    ctx = engine.Context(0)
    rng = np.random.default_rng(1)
    rows = []
    S, R = a.segments
    for cols in a.cols:
        for n in a.n:
            X = (rng.integers(0, 9, (n, cols)) / 8).astype(np.float32)
            rows.append(report(f"n={n} N={cols} K={a.k}", best(lambda: engine.knn_rows(ctx, X, a.k), 3 if n < 100000 else 1),
                               float(n) * n, cols))
        X = (rng.integers(0, 9, (S * R, cols)) / 8).astype(np.float32)
        seg = np.arange(S + 1) * R
        rows.append(report(f"{S} x {R} rows N={cols} K={a.k}", best(lambda: engine.knn_rows(ctx, X, a.k, seg)), float(S) * R * R, cols))
    out = dict(knn=rows)
    if a.layout:
        X = (rng.integers(0, 9, (a.layout, 8)) / 8).astype(np.float32)
        idx, d2 = engine.knn_rows(ctx, X, a.k)
        t0 = time.perf_counter()
        G = umap.fuzzy_graph(idx, d2, a.k)
        t1 = time.perf_counter()
        ab = umap.find_ab(1.0, 0.0)
        y = umap.layout(G, X, None, *ab)
        t2 = time.perf_counter()
        out["host"] = dict(n=a.layout, fuzzy_graph_s=round(t1 - t0, 3), layout_s=round(t2 - t1, 3), epochs=umap.default_epochs(a.layout),
                           finite=bool(np.isfinite(y).all()))
        print(f"host, n={a.layout}: fuzzy_graph {t1 - t0:.2f} s, layout ({out['host']['epochs']} epochs) {t2 - t1:.2f} s", flush=True)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
