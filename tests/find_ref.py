"""The pattern runs k_find_runs computes (panagram_amd/csrc/pg_find.hip), restated in numpy the obvious way.  No tests in
here: tests/test_find_cpu.py ties the restatement to scripts/query_index.py's literal expression and to hand-written cases,
tests/test_gpu_find.py holds the kernel to it."""
import numpy as np

from tests import rows_craft as rc


def ref_match(rows, n, stride, have, lack, min_have, max_lack):
    """the match bit of every sampled row (row j * stride) of ONE contig's rows; have / lack: column numbers"""
    bits = rc.unpack(np.asarray(rows, np.uint8)[::stride], n).astype(np.int64)  # 1. the first N bits
    nh = bits[:, sorted(set(have))].sum(axis=1)                                  # 2. the two column sums
    nl = bits[:, sorted(set(lack))].sum(axis=1)
    return (nh >= min_have) & (nl <= max_lack)


def ref_find_runs(rows, n, s, e, stride, have, lack, min_have, max_lack):
    """(starts, ends, matched) of the window [s, e) of sampled rows: the maximal runs [starts[i], ends[i]) of matching
    sampled rows, in sampled row numbers of the contig, and the number of matching rows"""
    s, e = int(s), int(e)
    m = ref_match(rows, n, stride, have, lack, min_have, max_lack)[s:e]
    d = np.diff(np.concatenate([[0], m.astype(np.int8), [0]]))                   # 3. the window's edges cut runs
    return np.flatnonzero(d == 1) + s, np.flatnonzero(d == -1) + s, int(m.sum())
