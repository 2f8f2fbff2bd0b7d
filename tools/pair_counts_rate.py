"""k_pair_counts on rows of real size, beside k_bin_colsums on the same rows and the host computation it replaces.

    python tools/pair_counts_rate.py [--rows 33554432] [--n 8 64 128] [--windows 350] [--only-gpu]

Per N: random rows planted on the GPU into a rows container of ``--rows`` rows (one contig; at N = 64 and 128 above the 256 MiB
Infinity Cache), then one window over all rows at stride 1 and ``--windows`` equal windows at stride 1 — pair_counts and, as
the yardstick, bin_colsums (no keep mask) on the same windows.  The times printed are host clocks around the synchronous
calls (allocation, launch, read-back of the matrices and the host's mirroring included; best of 3 after a warm call).  The
kernels' own times come from this script with ``--only-gpu`` (one warm and one timed call each, no host part) under
``rocprofv3 --kernel-trace --stats``.  Without ``--only-gpu`` it also times what the feature replaces: scipy's
``linkage(bitmap.T, "ward", "euclidean")`` on the viewer's sample of 50 000 rows at the same N, beside the linkage from
sqrt(H) of the pair counts.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from panagram_amd import engine  # noqa: E402

K = 21


def planted(ctx, n, rows, seed):
    """a rows container of one contig of ``rows`` random rows (bits past N zero), its statistics enqueued"""
    import torch
    nb = (n + 7) // 8
    ss = engine.SeqSet(ctx, [rows + K - 1])
    res = engine.AnchorResult.rows_container(ctx, K, n, ss, colsums=False)
    res._own_seqs = ss
    (ptr, size), _ = res.device_ptrs()
    assert size >= rows * nb

    class _Wrap:
        __cuda_array_interface__ = {"shape": (rows * nb,), "typestr": "|u1", "data": (ptr, False), "version": 3}

    buf = torch.as_tensor(_Wrap(), device=torch.device("cuda", ctx.device))
    gen = torch.Generator(device=buf.device).manual_seed(seed)
    step = 1 << 28
    for at in range(0, rows * nb, step):  # (in slices: randint's int64 temporaries)
        m = min(step, rows * nb - at)
        buf[at:at + m] = torch.randint(0, 256, (m,), generator=gen, device=buf.device, dtype=torch.int16).to(torch.uint8)
    if n % 8:
        buf.view(rows, nb)[:, -1] &= (1 << (n % 8)) - 1
    torch.cuda.synchronize()
    res.rows_epilogue()
    return res


def best(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        ts.append(time.perf_counter() - t0)
    return min(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 25)
    ap.add_argument("--n", type=int, nargs="+", default=[8, 64, 128])
    ap.add_argument("--windows", type=int, default=350)
    ap.add_argument("--only-gpu", action="store_true")
    a = ap.parse_args()
    ctx = engine.Context(0)
    out = dict(rows=a.rows, windows=a.windows, cases=[])
    reps = 1 if a.only_gpu else 3
    for n in a.n:
        nb = (n + 7) // 8
        res = planted(ctx, n, a.rows, 100 + n)
        per = a.rows // a.windows
        ws = np.arange(a.windows, dtype=np.uint64) * per
        we = ws + per
        we[-1] = a.rows
        zeros = np.zeros(a.windows, np.uint32)
        case = dict(n=n, row_bytes=nb, rows_mib=round(a.rows * nb / 2 ** 20, 1))
        t, one = best(lambda: res.pair_counts([0], [0], [a.rows]), reps)
        case["pairs_one_window_call_s"] = round(t, 5)
        t, many = best(lambda: res.pair_counts(zeros, ws, we), reps)
        case["pairs_windows_call_s"] = round(t, 5)
        t, (cs1, _) = best(lambda: res.bin_colsums([0], [0], [a.rows]), reps)
        case["colsums_one_window_call_s"] = round(t, 5)
        t, (csw, _) = best(lambda: res.bin_colsums(zeros, ws, we), reps)
        case["colsums_windows_call_s"] = round(t, 5)
        # at this size: the windows add up to the whole, the diagonal is the column sums, the matrix is symmetric
        case["windows_sum_to_whole"] = bool(np.array_equal(many.sum(axis=0), one[0]))
        case["diagonal_is_colsums"] = bool(np.array_equal(np.diagonal(one[0]), cs1[0]) and
                                           np.array_equal(np.diagonal(many, axis1=1, axis2=2), csw))
        case["symmetric"] = bool(np.array_equal(one[0], one[0].T))
        res.close()
        if not a.only_gpu:
            from scipy.cluster.hierarchy import linkage
            bits = (np.random.default_rng(n).random((50000, n)) < 0.5).astype(np.uint8)
            if n > 1:
                t0 = time.perf_counter()
                Z = linkage(bits.T, "ward", "euclidean")
                case["host_linkage_50000_rows_s"] = round(time.perf_counter() - t0, 4)
                b = bits.astype(np.int64)
                C = b.T @ b
                d = np.diag(C)
                H = d[:, None] + d[None, :] - 2 * C
                t0 = time.perf_counter()
                Z2 = linkage(np.sqrt(H[np.triu_indices(n, 1)].astype(np.float64)), method="ward")
                case["linkage_from_pair_counts_s"] = round(time.perf_counter() - t0, 5)
                case["linkages_equal"] = bool(np.array_equal(Z, Z2))
        out["cases"].append(case)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
