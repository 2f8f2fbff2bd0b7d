"""CPU: the numpy model of appending genomes to finished rows (tests/add_ref.py) against the oracle on the golden cases, and
what the crafted cases of tests/test_gpu_rows_append.py promise."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import add_ref as ar
from tests import helpers as H
from tests import rows_craft as rc

# (case, N_old): the splits tests/test_gpu_add_e2e.py adds through the index
GOLDEN_SPLITS = [("n2_k21", 1), ("n9_k21", 8), ("n9_k21", 7), ("n40_k31", 38), ("n65_k21", 64), ("n65_k21", 57), ("n40_k31", 29)]


@pytest.mark.parametrize("name, n_old", GOLDEN_SPLITS, ids=[f"{c}_{n}" for c, n in GOLDEN_SPLITS])
def test_model_append_of_oracle_rows_is_the_golden_payload(name, n_old):
    """the oracle's rows of the first N_old genomes + the remaining genomes' columns (out of the oracle's rows of the
    whole case) -> the golden bitmap.1 payload, and the statistics recomputed from the result are the oracle's"""
    fx = H.load_case(name)
    n, k = int(fx["ngenomes"]), int(fx["k"])
    dbs = H.case_dbs(fx)
    old_dbs = ar.restrict_dbs(dbs, n_old)
    for g in fx["anchors"]:
        fasta = fx[f"fasta_{g}"].tobytes()
        got, bins_rows, cs = [], [], np.zeros(n, np.int64)
        for _, seq in po.parse_fasta_cpp(fasta):
            old = po.anchor_contig(old_dbs, seq, k, n_old)[0]
            full, _, o_bins, _, o_cs = po.anchor_contig(dbs, seq, k, n)
            new = ar.append_rows(old, n_old, rc.unpack(full, n)[:, n_old:])
            assert np.array_equal(new, full)
            bins, colsums, low = rc.ref_stats(new, n, rc.bin_length(len(new)), 100)
            assert np.array_equal(bins, o_bins) and np.array_equal(colsums, o_cs) and np.array_equal(low, full[::100])
            got.append(new.tobytes())
        assert b"".join(got) == fx[f"a{g}_bitmap1"].tobytes()


def test_model_ignores_stale_bits_and_zeroes_the_rest():
    old = rc.with_pad_bits(rc.dense(50, 13, 1), 13)
    new = np.ones((50, 2), np.uint8)
    out = ar.append_rows(old, 13, new)
    bits = np.unpackbits(out, axis=1, bitorder="little")
    assert np.array_equal(bits[:, :13], rc.unpack(rc.dense(50, 13, 1), 13))
    assert bits[:, 13:15].all() and not bits[:, 15:].any()


def test_crafted_cases_cover_what_they_promise():
    from tests.add_ref import NKS, WIDTH_PAIRS
    wo = {(rc.row_bytes(a), rc.row_bytes(b)) for a, b in WIDTH_PAIRS}
    assert (1, 1) in wo and {(1, 2), (4, 5), (8, 9)} <= wo            # one byte on both sides; the widening steps
    words = {(rc.row_bytes(b) + 3) // 4 for _, b in WIDTH_PAIRS}                # words per new row: k_rows_append<1..5> ...
    assert words >= {1, 2, 3, 4, 5} and any(w > 5 for w in words)              # ... and <0>, word by word, beyond 160 genomes
    assert any(b > 160 and b - a > 8 for a, b in WIDTH_PAIRS)                  # (there with more new genomes than one block of 8)
    assert any(rc.row_bytes(b) > 16 for _, b in WIDTH_PAIRS)
    assert any(a % 8 == 0 for a, _ in WIDTH_PAIRS) and any(a % 8 for a, _ in WIDTH_PAIRS)
    for edge in (16, 64, 1024):                                         # a lane's positions, a slot, a tile
        assert {edge - 1, edge, edge + 1} <= set(NKS)
    assert 0 in NKS and any(nk > 2048 and nk % 1024 < 16 for nk in NKS)
    assert 0 < ar.SPLIT < len(NKS)
    for n_old, n_new in WIDTH_PAIRS:
        shapes = ar.block_shapes(n_old, n_new)
        assert {p for p, _, _ in shapes} & {1, 2, 8} and any(np_ == 2 and gap for _, np_, gap in shapes)
        assert any(per * nparts > n_new - n_old for per, nparts, _ in shapes)  # blocks wider than what they bring
        old, stale = ar.old_rows(n_old, False), ar.old_rows(n_old, True)
        new = ar.new_bits(n_old, n_new)
        assert [len(o) for o in old] == NKS and [b.shape for b in new] == [(nk, n_new - n_old) for nk in NKS]
        for o, s, b in zip(old, stale, new):
            if n_old % 8 and len(o):
                assert not np.array_equal(o, s)                         # the stale bits are there ...
            assert np.array_equal(ar.append_rows(o, n_old, b), ar.append_rows(s, n_old, b))  # ... and do not count
            if len(o):
                assert rc.unpack(ar.append_rows(o, n_old, b), n_new)[-1, n_new - 1] == 1  # the last row's highest bit


def test_column_blocks_are_the_oracle_layout():
    """blocks cut out of the model's rows by the oracle's extract_columns equal the blocks the GPU test uploads, gaps apart"""
    tile = 1024
    n_old, n_new = 15, 17
    new = ar.new_bits(n_old, n_new)
    rows = [ar.append_rows(o, n_old, b) for o, b in zip(ar.old_rows(n_old, False), new)]
    for per, nparts, gap in ar.block_shapes(n_old, n_new):
        blob, stride = ar.column_blocks(new, nparts, per, tile, gap_words=gap, fill=0xFF)
        for i in range(nparts):
            want = po.extract_columns(rows, n_new, n_old + i * per, per, tile=tile)
            assert np.array_equal(blob[i * stride:i * stride + len(want)], want)
            assert (blob[i * stride + len(want):(i + 1) * stride] == 0xFF).all() and stride == len(want) + 8 * gap
