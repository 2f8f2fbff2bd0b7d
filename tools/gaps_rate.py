"""k_absence_runs on rows of real size, beside the route to the same runs without it: N calls of find_runs with lack = {g}.

    python tools/gaps_rate.py [--cases 8:100000000 64:20000000] [--reps 5] [--only-gpu]

Per case N:rows, rows planted on the GPU into a rows container of one contig, two patterns:
  variants  every row holds every genome, but for runs of k = 21 absent rows planted in every column at one start in 1000 (what
            substitutions at a rate of 1e-3 leave; runs that touch merge into longer ones)
  dense     random rows: every other row starts or ends a run in every column — the most work the column walk can get
One window over all rows at stride 1.  Three calls on it: absence_runs without emission (the spectrum, the absent rows and the
edges alone), absence_runs with min_len = k - 1 (the candidates written, sorted and read back), and find_runs once per genome.
The times printed are host clocks around the synchronous calls (allocation, launch, the stitch on the host and the read-back
included; the median of --reps after a warm call).  The kernels' own times come from this script with ``--only-gpu`` (one warm
and one timed call each, no find_runs) under ``rocprofv3 --kernel-trace --stats``.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from panagram_amd import engine  # noqa: E402

K = 21


def planted(ctx, n, rows, seed, pattern):
    """a rows container of one contig of ``rows`` rows of the pattern (bits past N zero), its statistics enqueued"""
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
    if pattern == "variants":
        buf.fill_(0xFF)
        v = buf.view(rows, nb)
        for g in range(n):
            at = torch.randint(0, rows - K, (rows // 1000,), generator=gen, device=buf.device)
            for off in range(K):
                v[at + off, g // 8] &= 0xFF ^ (1 << (g % 8))  # (equal indices write equal bytes)
    else:
        step = 1 << 28
        for at in range(0, rows * nb, step):  # (in slices: randint's int64 temporaries)
            m = min(step, rows * nb - at)
            buf[at:at + m] = torch.randint(0, 256, (m,), generator=gen, device=buf.device, dtype=torch.int16).to(torch.uint8)
    if n % 8:
        buf.view(rows, nb)[:, -1] &= (1 << (n % 8)) - 1
    torch.cuda.synchronize()
    res.rows_epilogue()
    return res


def median(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


def words(n, cols):
    w = np.zeros((n + 31) // 32, np.uint32)
    for g in cols:
        w[g // 32] |= np.uint32(1 << (g % 32))
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["8:100000000", "64:20000000"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-gpu", action="store_true")
    a = ap.parse_args()
    ctx = engine.Context(0)
    out = dict(chunk=engine.GAPS_CHUNK, k=K, cases=[])
    reps = 1 if a.only_gpu else a.reps
    for spec in a.cases:
        n, rows = (int(x) for x in spec.split(":"))
        nb = (n + 7) // 8
        for pattern in ("variants", "dense"):
            res = planted(ctx, n, rows, 100 + n, pattern)
            w = ([0], [0], [rows])
            case = dict(n=n, rows=rows, pattern=pattern, row_bytes=nb, rows_mb=round(rows * nb / 1e6, 1))
            t, (_, hist, absent, edges) = median(lambda: res.absence_runs(*w, None, 4 * K, emit=False), reps)
            case["spectrum_call_s"] = round(t, 5)
            case["spectrum_gb_per_s"] = round(rows * nb / t / 1e9, 1)
            t, (runs, hist2, _, _) = median(lambda: res.absence_runs(*w, None, 4 * K, min_len=K - 1), reps)
            case["emit_call_s"] = round(t, 5)
            case["emit_gb_per_s"] = round(rows * nb / t / 1e9, 1)
            case["closed_runs"] = int(hist.sum())
            case["emitted_runs"] = int(len(runs))
            case["absent_rows"] = int(absent.sum())
            # at this size: the two calls agree, the emitted runs are the spectrum's bins from k - 1 on, sorted by (genome, row)
            case["calls_agree"] = bool(np.array_equal(hist, hist2) and len(runs) == int(hist[:, :, K - 1:].sum()))
            case["sorted"] = bool((np.diff(runs[:, 1] * (rows + 1) + runs[:, 2]) > 0).all())
            if not a.only_gpu:
                none = words(n, [])

                def by_find():
                    return [res.find_runs(*w, none, words(n, [g]), 0, 0)[0] for g in range(n)]
                t, per = median(by_find, max(1, reps // 2))
                case["find_runs_n_calls_s"] = round(t, 5)
                # the same runs: find's are cut by the window's edges only, so all but a column's open runs are the closed ones
                closed = sum(len(r) for r in per) - int((edges[0] > 0).sum())
                case["find_agrees"] = bool(closed == int(hist.sum()) and sum(int((r[:, 2] - r[:, 1]).sum()) for r in per) == int(absent.sum()))
            res.close()
            out["cases"].append(case)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
