"""k_pattern_counts on rows of real size, beside the count launch of k_find_runs on the same window: the count launch reads
every sampled row once and writes 16 bytes per chunk — this tree's measured yardstick for one pass over rows; the spectrum reads
them once too, then hashes every run head into LDS and flushes each chunk's table with global atomics.

    python tools/patterns_rate.py [--rows 100000000] [--reps 5] [--only-gpu]

Row sets, planted on the GPU into a rows container of ``--rows`` rows (one contig, one window over all of it, stride 1):
  synth N d   the rows an N-genome synthetic index gives at substitution rate d (tools/_synth.py's model): genome 0 is the
              anchor and holds every k-mer, genome g holds the k-mer at position p iff it has no substitution in [p, p + 21).
              Equal neighbouring rows come in runs; ``heads_per_row`` is the share of rows that differ from the row before.
  dense 64    random 8-byte rows: every row distinct — no call can hold the spectrum, and pattern_counts raises after its
              last retry (the cliff a user should know about)
Per row set: (a) find_counts (rule "genome 0 holds it"), (b) pattern_counts with its retries, (c) the one pattern call whose
capacity sufficed.  Times are device events on the stream the context was pointed at, around the synchronous calls (copies,
memsets, the table's download and the host's sort included; a warm call, then the median and the least of ``--reps``).  The
kernels' own times come from this script with ``--only-gpu`` (one warm and one timed call each) under
``rocprofv3 --kernel-trace --stats``.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from panagram_amd import engine  # noqa: E402

K = 21


def container(ctx, n, rows):
    import torch
    nb = (n + 7) // 8
    ss = engine.SeqSet(ctx, [rows + K - 1])
    res = engine.AnchorResult.rows_container(ctx, K, n, ss, colsums=False)
    res._own_seqs = ss
    (ptr, size), _ = res.device_ptrs()
    assert size >= rows * nb

    class _Wrap:
        __cuda_array_interface__ = {"shape": (rows * nb,), "typestr": "|u1", "data": (ptr, False), "version": 3}

    return res, torch.as_tensor(_Wrap(), device=torch.device("cuda", ctx.device)).view(rows, nb)


def plant_synth(buf, n, d, seed):
    """bit g of row p: genome g has no substitution in positions [p, p + K); genome 0 has none at all"""
    import torch
    rows, nb = buf.shape
    gen = torch.Generator(device=buf.device).manual_seed(seed)
    buf.zero_()
    for g in range(n):
        if g == 0:
            held = torch.ones(rows, dtype=torch.uint8, device=buf.device)
        else:
            hit = torch.rand(rows + K - 1, generator=gen, device=buf.device) < d
            c = torch.zeros(rows + K, dtype=torch.int32, device=buf.device)
            c[1:] = torch.cumsum(hit, 0, dtype=torch.int32)
            held = (c[K:] == c[:rows]).to(torch.uint8)
        buf[:, g // 8] |= held << (g % 8)


def plant_dense(buf, seed):
    import torch
    gen = torch.Generator(device=buf.device).manual_seed(seed)
    flat = buf.view(-1)
    step = 1 << 28
    for at in range(0, flat.numel(), step):  # (in slices: randint's temporaries)
        m = min(step, flat.numel() - at)
        flat[at:at + m] = torch.randint(0, 256, (m,), generator=gen, device=buf.device, dtype=torch.int16).to(torch.uint8)


def timed(stream, f, reps):
    """(median ms, least ms, what f returned) by device events on ``stream`` around the synchronous call, after a warm call"""
    import torch
    f()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        out = f()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return round(statistics.median(ms), 3), round(min(ms), 3), out


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-gpu", action="store_true")
    a = ap.parse_args()
    reps = 1 if a.only_gpu else a.reps
    ctx = engine.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    out = dict(rows=a.rows, chunk=engine.PATTERN_CHUNK, find_chunk=engine.FIND_CHUNK, first_cap=engine.PATTERN_FIRST_CAP,
               max_cap=engine.PATTERN_MAX_CAP, cases=[])
    for name, n, d in [("synth", 8, 0.01), ("synth", 64, 0.01), ("synth", 64, 0.001), ("dense", 64, None)]:
        res, buf = container(ctx, n, a.rows)
        if name == "synth":
            plant_synth(buf, n, d, 100 + n)
        else:
            plant_dense(buf, 7)
        heads = 1 + int((buf[1:] != buf[:-1]).any(dim=1).sum())
        torch.cuda.synchronize()
        res.rows_epilogue()
        ctx.synchronize()
        case = dict(rows_set=name, n=n, d=d, row_bytes=buf.shape[1], rows_mib=round(buf.numel() / 2 ** 20, 1),
                    heads_per_row=round(heads / a.rows, 4))
        win = ([0], [0], [a.rows])
        hw = np.array([1] + [0] * ((n + 31) // 32 - 1), np.uint32)
        case["find_count_ms"], case["find_count_min_ms"], (_, matched) = timed(stream, lambda: res.find_counts(*win, hw, None, 1, 0), reps)

        def spectrum():
            try:
                return res.pattern_counts(*win)
            except ValueError as e:
                return str(e)
        case["patterns_ms"], case["patterns_min_ms"], got = timed(stream, spectrum, reps)
        if isinstance(got, str):
            case["patterns_raised"] = got
        else:
            keys, counts = got
            cap, calls = engine.PATTERN_FIRST_CAP, 1
            while cap < len(keys):  # (pattern_counts' own ladder)
                cap, calls = min(cap * 16, engine.PATTERN_MAX_CAP), calls + 1
            case.update(distinct=len(keys), calls=calls, last_cap=cap)
            case["patterns_last_call_ms"], case["patterns_last_call_min_ms"], _ = timed(
                stream, lambda: res._patterns(*win, None, 1, 1, cap), reps)
            # at this size: the counts add up to the rows, genome 0's rows are the find rule's matching rows, the keys ascend
            held0 = int(counts[(keys & np.uint64(1)) == 1].sum())
            case["conserved"] = bool(int(counts.sum()) == a.rows and held0 == int(matched[0]) and (keys[1:] > keys[:-1]).all())
            case["patterns_over_find_count"] = round(case["patterns_last_call_ms"] / case["find_count_ms"], 2)
        res.close()
        del buf
        out["cases"].append(case)
    ctx.set_stream(None)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
