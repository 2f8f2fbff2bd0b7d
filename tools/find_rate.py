"""k_find_runs on rows of real size, beside k_bin_colsums (no mask) on the same rows: the two passes of the pattern search
read every row twice, the column sums once.

    python tools/find_rate.py [--rows 33554432] [--n 8 64 128] [--windows 350] [--only-gpu]

Per N and pattern: rows planted on the GPU into a rows container of ``--rows`` rows (one contig; at N = 64 and 128 above the
256 MiB Infinity Cache), then one window over all rows at stride 1 and ``--windows`` equal windows at stride 1.
  dense    random rows, the rule "genome 0 holds it, genome 1 does not" (N = 1: genome 0 holds it): a quarter of the rows match
  checker  0xAA / 0x55 rows, the rule "genome 0 holds it": every other row starts a run — the most runs rows can give
Three calls on each window set: find_counts (the count launch alone), find_runs (count, emit, and the runs read back to the
host: 8 bytes per run) and, as the yardstick, bin_colsums.  The times printed are host clocks around the synchronous calls
(allocation, launches, read-back included; best of 3 after a warm call).  The kernels' own times come from this script with
``--only-gpu`` (one warm and one timed call each) under ``rocprofv3 --kernel-trace --stats``.  Prints one JSON line."""
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
    if pattern == "checker":
        v = buf.view(rows, nb)
        v[0::2] = 0xAA
        v[1::2] = 0x55
    else:
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


def words(n, cols):
    w = np.zeros((n + 31) // 32, np.uint32)
    for g in cols:
        w[g // 32] |= np.uint32(1 << (g % 32))
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 25)
    ap.add_argument("--n", type=int, nargs="+", default=[8, 64, 128])
    ap.add_argument("--windows", type=int, default=350)
    ap.add_argument("--only-gpu", action="store_true")
    a = ap.parse_args()
    ctx = engine.Context(0)
    out = dict(rows=a.rows, windows=a.windows, chunk=engine.FIND_CHUNK, cases=[])
    reps = 1 if a.only_gpu else 3
    per = a.rows // a.windows
    ws = np.arange(a.windows, dtype=np.uint64) * per
    we = ws + per
    we[-1] = a.rows
    zeros = np.zeros(a.windows, np.uint32)
    for n in a.n:
        nb = (n + 7) // 8
        for pattern in ("dense", "checker"):
            res = planted(ctx, n, a.rows, 100 + n, pattern)
            hw = words(n, [0])
            lw = words(n, [1] if pattern == "dense" and n > 1 else [])
            rule = (hw, lw, 1, 0)
            case = dict(n=n, pattern=pattern, row_bytes=nb, rows_mib=round(a.rows * nb / 2 ** 20, 1))
            t, (nr1, m1) = best(lambda: res.find_counts([0], [0], [a.rows], *rule), reps)
            case["count_one_window_call_s"] = round(t, 5)
            t, (nrw, mw) = best(lambda: res.find_counts(zeros, ws, we, *rule), reps)
            case["count_windows_call_s"] = round(t, 5)
            t, (runs1, _) = best(lambda: res.find_runs([0], [0], [a.rows], *rule), reps)
            case["runs_one_window_call_s"] = round(t, 5)
            t, (runsw, _) = best(lambda: res.find_runs(zeros, ws, we, *rule), reps)
            case["runs_windows_call_s"] = round(t, 5)
            t, (cs1, _) = best(lambda: res.bin_colsums([0], [0], [a.rows]), reps)
            case["colsums_one_window_call_s"] = round(t, 5)
            t, (csw, _) = best(lambda: res.bin_colsums(zeros, ws, we), reps)
            case["colsums_windows_call_s"] = round(t, 5)
            case["runs"] = int(nr1[0])
            case["matched"] = int(m1[0])
            # at this size: the windows' matching rows add up to the whole's; a window's edge cuts at most one run in two; the
            # runs hold the matching rows; with genome 1 out of the rule the matching rows are genome 0's column sum
            case["windows_sum_to_whole"] = bool(mw.sum() == m1[0] and 0 <= int(nrw.sum()) - int(nr1[0]) < a.windows)
            case["runs_hold_matched"] = bool(len(runs1) == nr1[0] and (runs1[:, 2] - runs1[:, 1]).sum() == m1[0] and
                                             len(runsw) == nrw.sum() and (runsw[:, 2] - runsw[:, 1]).sum() == m1[0])
            case["sorted"] = bool((runs1[1:, 1] > runs1[:-1, 2]).all())
            if pattern == "checker":
                case["matched_is_colsum"] = bool(m1[0] == cs1[0, 0] and np.array_equal(mw, csw[:, 0]))
                case["every_other_row"] = bool(nr1[0] == a.rows // 2)
            res.close()
            out["cases"].append(case)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
