"""The numpy model of selecting columns out of finished bitmap rows (k_rows_select*, pg_result_select_columns_range) and the
crafted cases its GPU test runs.  No tests in here: tests/test_subset_cpu.py holds the model to the oracle on the golden
cases and proves what the crafted cases promise, tests/test_gpu_rows_select.py holds the kernels to the model.

The model: bit j of a new row is bit sel[j] of the old one — ``unpackbits(old)[:, :N_old][:, sel]`` ->
``packbits(bitorder="little")``.  Bits at and past N_old of the old rows' last byte do not count; bits at and past N_new of
the new rows are zero."""
import numpy as np

from tests import add_ref as ar
from tests import rows_craft as rc


def select_rows(old_rows, n_old, sel):
    """(nk, ceil(N_old / 8)) uint8 rows -> (nk, ceil(len(sel) / 8)) uint8 rows"""
    return rc.pack(rc.unpack(old_rows, n_old)[:, np.asarray(sel, np.int64)])


def segments(sel):
    """the host's segment compiler (csrc/pg_select_host.h: select_segments) restated: (src_bit, dst_bit, len) of every maximal
    run of consecutive source bits going to consecutive destination bits, cut at the destination's 32-bit words"""
    out, j, n = [], 0, len(sel)
    while j < n:
        ln = 1
        while j + ln < n and (j + ln) % 32 and sel[j + ln] == sel[j] + ln:
            ln += 1
        out.append((int(sel[j]), j, ln))
        j += ln
    return out


def kernel_form(n_old):
    """which kernel launch_rows_select takes: "b1" (one-byte rows on both sides), the words per source row 1..5 of the
    template instances, 0 for the word-by-word form beyond them"""
    if n_old <= 8:
        return "b1"
    nws = (rc.row_bytes(n_old) + 3) // 4
    return nws if nws <= 5 else 0


def needed_words(sel):
    """the source words some segment reads (select_needed_words)"""
    need = set()
    for s, _, ln in segments(sel):
        need.add(s // 32)
        if s % 32 + ln > 32:
            need.add(s // 32 + 1)
    return need


# ---------------------------------------------------------------------------
# the crafted cases
# ---------------------------------------------------------------------------
# (N_old, N_new): one byte on both sides (k_rows_select_b1); the byte-count steps 2 -> 1, 3 -> 2, 5 -> 4, 9 -> 8 bytes and
# 40 -> 38 genomes; 64 -> 8 (a source word no segment reads); 100 -> 96, 129 -> 128 and 130 -> 129 (with the rest: 1..5 words per
# source row, <1>..<5>, and 1..5 words per destination row); 161 -> 160 and 170 -> 161, the word-by-word form <0> (six words
# per destination row at 161); 16 -> 16 and 33 -> 33, permutations
WIDTH_PAIRS = [(8, 7), (8, 1), (9, 8), (17, 16), (33, 32), (65, 64), (40, 38), (64, 8), (100, 96), (129, 128), (130, 129), (161, 160),
               (170, 161), (16, 16), (33, 33)]
NKS = ar.NKS  # the edges of a lane's 16 positions, of a slot of 64 and of a tile of 1024
SPLIT = 7     # the destination is filled in two source batches: contigs [0, SPLIT) and [SPLIT, len(NKS))


def selections(n_old, n_new):
    """[(name, sel)] of one width pair.  Every sel has N_new entries but "one", which keeps a single column (a destination
    of one genome).  With m = N_old - N_new columns to drop: the first m, the last m, m in the middle, m from column 31 on
    and m from column 32 on (the two sides of a 32-bit boundary, where the source has them); every other column (the even
    ones, then as many odd ones as it takes); the middle selection in descending order (N_new = N_old: the full reversal); a
    shuffle."""
    m = n_old - n_new
    every = np.arange(n_old)

    def drop(at):
        return np.concatenate([every[:at], every[at + m:]])
    out = [("first", drop(0)), ("last", drop(n_new)), ("middle", drop(n_new // 2))]
    for at in (31, 32):
        if m and at + m <= n_old:
            out.append((f"at{at}", drop(at)))
    out.append(("alternate", np.concatenate([every[::2], every[1::2]])[:n_new]))
    out.append(("one", np.array([n_old - 1])))
    out.append(("reversed", drop(n_new // 2)[::-1]))
    out.append(("shuffle", np.random.default_rng(1000 * n_old + n_new).permutation(n_old)[:n_new]))
    return [(name, np.asarray(sel, np.uint32)) for name, sel in out]


def old_rows(n_old, stale):
    """one (nk, W_old) array per contig of NKS (tests/add_ref.py: dense rows, rows of ones, the last column alone);
    ``stale``: the bits at and past N_old of the last byte set"""
    return ar.old_rows(n_old, stale)
