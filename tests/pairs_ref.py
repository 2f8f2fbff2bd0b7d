"""The pair counts k_pair_counts computes (panagram_amd/csrc/pg_pairs.hip), restated in numpy.  No tests in here:
tests/test_pair_counts_cpu.py ties the restatement to the column sums of tests/rows_craft.py and holds the host side to
it, tests/test_gpu_pair_counts.py the kernel."""
import numpy as np

from tests import rows_craft as rc


def ref_pair_counts(rows, n, start, end, stride):
    """[N, N] int64: entry (a, b) = sampled rows [start, end) of ONE contig's (nk, nbytes) rows — sampled row j is row
    j * stride — holding both bit a and bit b, of their first N bits: B.T @ B of those rows as 0/1"""
    B = rc.unpack(np.asarray(rows, np.uint8)[::stride][int(start):int(end)], n).astype(np.int64)
    return B.T @ B
