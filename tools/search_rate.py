"""k_presence_profile on rows of real size beside k_absence_runs on the same rows, and the shares of a whole search.

    python tools/search_rate.py [--cases 8:100000000 64:100000000] [--reps 5] [--only-gpu] [--queries 50000] [--query-len 1500]

Per case N:rows, rows planted on the GPU into a rows container of one contig (tools/gaps_rate.py's VARIANTS pattern: every row
holds every genome, but for runs of k = 21 absent rows planted in every column at one start in 1000 — what a query that the
genomes carry with substitutions at a rate of 1e-3 leaves).  Two window sets over them: ONE window of all rows, and rows / 1000
windows of 1000 rows (a window per gene: one chunk each).  Two calls on each: presence_profile, and absence_runs with maxlen = 84
and no emission — the call one would have to make without k_presence_profile.  The times printed are host clocks around the
synchronous calls (chunk table, upload, launch, read-back and the stitch on the host included; the median of --reps after a warm
call); the kernels' own times come from this script with ``--only-gpu`` (one warm and one timed call each, no search) under
``rocprofv3 --kernel-trace --stats``.  At this size the two kernels must agree: hits = rows - absent rows, and covered = hits +
the spectrum's runs clipped to k - 1 + (k - 1 where a row is held).

Then a search as Index.search makes it: a table of 8 synthetic genomes (--mb each, 1 % apart), --queries records of --query-len
bases cut from them as FASTA text; SeqSet.from_fasta, a rows-only AnchorResult, run() and presence_profile over every record.
Prints k_probe's time (AnchorResult.timing(), HIP events) beside the host clock of each step.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _synth as po  # noqa: E402
from gaps_rate import K, median, planted  # noqa: E402
from panagram_amd import engine  # noqa: E402

MAXLEN = 84


def search_leg(ctx, mb, nq, qlen, reps):
    L, G = int(mb * 1e6), 8
    gen = po.synth_genomes(G, [L], 0.01, 4321)
    tbl = engine.PanTable(ctx, K, G, expected_keys=int(L * 2.5))
    for g in range(G):
        ss = engine.SeqSet.from_host(ctx, [po.codes_to_ascii(gen[g][0])])
        tbl.insert_seqset(g, ss)
        ss.close()
    tbl.rehash(2.0)
    rng = np.random.default_rng(9)
    at = rng.integers(0, L - qlen, nq)
    text = b"".join(b">q%d\n%s\n" % (i, po.codes_to_ascii(gen[i % G][0][a:a + qlen])) for i, a in enumerate(at))
    contigs, starts, ends = np.arange(nq), np.zeros(nq, np.uint64), np.full(nq, qlen - K + 1, np.uint64)
    steps = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        ss = engine.SeqSet.from_fasta(ctx, text)
        t1 = time.perf_counter()
        res = engine.AnchorResult(tbl, ss, colsums=False, rows_only=True)
        res.run()
        ctx.synchronize()
        t2 = time.perf_counter()
        prof, rows = res.presence_profile(contigs, starts, ends)
        t3 = time.perf_counter()
        probe_ms = res.timing()[0]
        res.close()
        ss.close()
        steps.append((t1 - t0, t2 - t1, t3 - t2, probe_ms / 1e3))
    pack, anchor, profile, probe = (float(np.median([s[i] for s in steps[1:]])) for i in range(4))
    tbl.close()
    hits = prof[:, :, 0].astype(np.int64)
    return dict(genomes=G, genome_mb=mb, queries=nq, query_len=qlen, fasta_mb=round(len(text) / 1e6, 1),
                from_fasta_s=round(pack, 5), result_and_run_s=round(anchor, 5), k_probe_s=round(probe, 6),
                presence_profile_call_s=round(profile, 5), whole_s=round(pack + anchor + profile, 5),
                k_probe_share=round(probe / (pack + anchor + profile), 3),
                own_genome_whole=bool((hits[np.arange(nq), np.arange(nq) % G] == qlen - K + 1).all()),
                mean_frac=round(float(hits.mean() / (qlen - K + 1)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["8:100000000", "64:100000000"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-gpu", action="store_true")
    ap.add_argument("--mb", type=float, default=20.0)
    ap.add_argument("--queries", type=int, default=50000)
    ap.add_argument("--query-len", type=int, default=1500)
    a = ap.parse_args()
    ctx = engine.Context(0)
    out = dict(chunk=engine.PROFILE_CHUNK, k=K, maxlen=MAXLEN, cases=[])
    reps = 1 if a.only_gpu else a.reps
    for spec in a.cases:
        n, rows = (int(x) for x in spec.split(":"))
        nb = (n + 7) // 8
        res = planted(ctx, n, rows, 100 + n, "variants")
        nwin = rows // 1000
        sets = {"one_window": ([0], [0], [rows]),
                "windows_of_1000": (np.zeros(nwin, np.uint32), np.arange(nwin, dtype=np.uint64) * 1000, np.arange(1, nwin + 1, dtype=np.uint64) * 1000)}
        for name, w in sets.items():
            case = dict(n=n, rows=rows, windows=name, nwin=len(w[0]), row_bytes=nb, rows_mb=round(rows * nb / 1e6, 1))
            t, (prof, allnone) = median(lambda: res.presence_profile(*w), reps)
            case["profile_call_s"] = round(t, 5)
            case["profile_rows_per_s"] = round(rows / t / 1e9, 2)  # (G rows/s)
            t, (_, hist, absent, _) = median(lambda: res.absence_runs(*w, None, MAXLEN, emit=False), reps)
            case["absence_runs_call_s"] = round(t, 5)
            case["absence_runs_rows_per_s"] = round(rows / t / 1e9, 2)
            prof, absent = prof.astype(np.int64), absent.astype(np.int64)
            length = (np.asarray(w[2], np.int64) - np.asarray(w[1], np.int64))[:, None]
            some = prof[:, :, 0] > 0
            # (the spectrum of 10^5 windows x 64 genomes is 4.4 GB on the host: no copy of it is made here)
            clipped = (hist @ np.minimum(np.arange(MAXLEN + 1), K - 1).astype(np.uint64)).astype(np.int64)
            case["kernels_agree"] = bool(np.array_equal(prof[:, :, 0], length - absent) and
                                         np.array_equal(prof[:, :, 5], prof[:, :, 0] + clipped + (K - 1) * some) and
                                         np.array_equal(prof[:, :, 1], hist.sum(axis=2).astype(np.int64) + some))
            case["hits"] = int(prof[:, :, 0].sum())
            case["rows_all"] = int(allnone[:, 0].sum())
            out["cases"].append(case)
        res.close()
    if not a.only_gpu:
        out["search"] = search_leg(ctx, a.mb, a.queries, a.query_len, max(1, a.reps // 2))
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
