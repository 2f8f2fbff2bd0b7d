"""A numpy restatement of the pattern spectrum (panagram_amd/csrc/pg_patterns.hip's header): unpack the rows, take the selected
columns and the sampled rows of each window, np.unique the packed keys.  No tests in here: tests/test_patterns_cpu.py ties it to
DataFrame.value_counts(), tests/test_gpu_pattern_counts.py holds the kernel to it."""
import numpy as np

from tests import rows_craft as rc


def ref_keys(rows, n, stride, select):
    """uint64 key of every sampled row (row j * stride) of ONE contig's (nk, nbytes) rows: bit i of the key is the row's bit
    for the i-th of the sorted ``select`` columns"""
    cols = sorted(int(g) for g in select)
    assert 1 <= len(cols) <= 64 and len(set(cols)) == len(cols) and 0 <= cols[0] and cols[-1] < n
    bits = rc.unpack(np.asarray(rows, np.uint8)[::stride], n)[:, cols]
    packed = np.packbits(bits, axis=1, bitorder="little")  # (nk, ceil(m / 8)): byte b holds key bits 8b .. 8b + 7
    wide = np.zeros((len(packed), 8), np.uint8)
    wide[:, :packed.shape[1]] = packed
    return wide.view("<u8").reshape(-1)


def ref_pattern_counts(rows_per_contig, n, contigs, starts, ends, stride, select):
    """(keys ascending, counts, sampled rows): the spectrum over all windows together — window i = sampled rows
    [starts[i], ends[i]) of contig contigs[i]"""
    keys = [ref_keys(r, n, stride, select) for r in rows_per_contig]
    taken = [keys[int(c)][int(s):int(e)] for c, s, e in zip(contigs, starts, ends)]
    for t, s, e in zip(taken, starts, ends):
        assert len(t) == int(e) - int(s)  # every window inside its contig
    allk = np.concatenate(taken) if taken else np.zeros(0, np.uint64)
    k, c = np.unique(allk, return_counts=True)
    return k.astype(np.uint64), c.astype(np.uint64), len(allk)
