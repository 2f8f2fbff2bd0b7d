"""The numpy model of appending genomes to finished bitmap rows (k_rows_append*, pg_result_append_columns_range) and the
crafted cases its GPU test runs.  No tests in here: tests/test_add_cpu.py holds the model to the oracle on the golden
cases and proves what the crafted cases promise, tests/test_gpu_rows_append.py holds the kernels to the model.

The model: the first N_old bits of every old row, then the new genomes' bit columns, packed little-endian —
``unpackbits(old)[:, :N_old]`` ++ new columns -> ``packbits(bitorder="little")``.  Bits at and past N_old of the old rows'
last byte do not count; bits at and past N_new of the new rows are zero."""
import numpy as np

from oracle import pyoracle as po
from tests import rows_craft as rc


def append_rows(old_rows, n_old, new_bits):
    """(nk, ceil(N_old / 8)) uint8 rows + (nk, m) 0/1 columns -> (nk, ceil((N_old + m) / 8)) uint8 rows"""
    new_bits = np.asarray(new_bits, np.uint8)
    bits = np.concatenate([rc.unpack(old_rows, n_old), new_bits], axis=1)
    return rc.pack(bits)


def restrict_dbs(dbs, n):
    """the oracle's 32-genome databases cut to the first n genomes (a key none of them holds keeps an empty mask)"""
    out = []
    for d, (keys, masks) in enumerate(dbs[:(n + 31) // 32]):
        left = min(32, n - 32 * d)
        out.append((keys, masks & np.uint32(0xFFFFFFFF if left >= 32 else (1 << left) - 1)))
    return out


def column_blocks(new_bits_per_contig, nparts, per, tile, gap_words=0, fill=0):
    """the new genomes' columns as the kernels read them: ``nparts`` blocks of ``per`` genomes each in the layout of
    oracle.pyoracle.extract_columns (block i = columns i * per .. of ``new_bits_per_contig``, (nk, m) 0/1 per contig;
    columns past m are zero), ``gap_words`` u64 of ``fill`` bytes behind every block.  Returns (bytes, block stride in bytes)."""
    blocks = []
    for i in range(nparts):
        rows = []
        for nb in new_bits_per_contig:
            part = np.zeros((len(nb), per), np.uint8)
            have = np.asarray(nb, np.uint8)[:, i * per:(i + 1) * per]
            part[:, :have.shape[1]] = have
            rows.append(rc.pack(part))
        blk = po.extract_columns(rows, per, 0, per, tile=tile)
        blocks.append(np.concatenate([blk, np.full(8 * gap_words, fill, np.uint8)]))
    return np.concatenate(blocks), len(blocks[0])


# ---------------------------------------------------------------------------
# the crafted cases
# ---------------------------------------------------------------------------
# (N_old, N_new): one byte -> one byte (k_rows_append_b1), every number of words per new row of the general kernel
# (1..5 words: <1>..<5>; 96 -> 100 is the pair with 4), the widening steps 1 -> 2, 4 -> 5, 8 -> 9 bytes, rows wider than 16
# bytes, and beyond 160 genomes the word-by-word form <0> (160 -> 161: 20 -> 21 bytes, six words; 161 -> 170: 21 -> 22)
WIDTH_PAIRS = [(1, 2), (7, 8), (8, 9), (8, 16), (9, 16), (15, 17), (31, 33), (32, 33), (38, 40), (63, 64), (64, 65), (65, 73), (120, 129),
               (96, 100), (160, 161), (161, 170)]
# k-mers per contig of the one sequence set: on each side of a lane's 16 positions (one-byte rows), of a wave's slot of 64
# and of a tile of 1024; an empty contig; a last tile of 7 positions behind two whole ones
NKS = [0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 2049 + 7]
# (per, nparts, gap in u64 between blocks): blocks wider than the genomes they bring are allowed (their other columns are zero)
BLOCK_SHAPES = [(1, 1, 0), (2, 1, 0), (8, 1, 0), (1, 2, 3), (2, 2, 5), (8, 2, 1)]
SPLIT = 7  # the destination is filled in two source batches: contigs [0, SPLIT) and [SPLIT, len(NKS))


def block_shapes(n_old, n_new):
    """the block shapes that can bring n_new - n_old genomes"""
    return [(per, nparts, gap) for per, nparts, gap in BLOCK_SHAPES if per * nparts >= n_new - n_old]


def old_rows(n_old, stale):
    """one (nk, W_old) array per contig of NKS: dense rows, columns and rows of ones; ``stale``: the bits at and past
    N_old of the last byte set, as a file from elsewhere might hold them"""
    out = []
    for ci, nk in enumerate(NKS):
        r = rc.back_to_back(nk, [(2, lambda m: rc.dense(m, n_old, 100 + ci)), (1, lambda m: rc.ones(m, n_old)),
                                 (1, lambda m: rc.column(m, n_old, n_old - 1))]) if nk else rc.zeros(0, n_old)
        out.append(rc.with_pad_bits(r, n_old) if stale else r)
    return out


def new_bits(n_old, n_new):
    """one (nk, m) 0/1 array per contig: the first new genome dense, the last one present everywhere (the very last row's
    highest bit is set), the others every third row"""
    m = n_new - n_old
    out = []
    for ci, nk in enumerate(NKS):
        b = np.zeros((nk, m), np.uint8)
        b[:, 0] = np.random.default_rng(500 + ci).random(nk) < 0.5
        if m > 1:
            b[:, 1:] = (np.arange(nk) % 3 == 0)[:, None]
            b[:, m - 1] = 1
        if nk:
            b[-1, m - 1] = 1
        out.append(b)
    return out
