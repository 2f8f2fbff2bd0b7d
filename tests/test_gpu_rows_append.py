"""GPU: appending genomes to finished rows (AnchorResult.append_columns: k_rows_append_b1 for one-byte rows on both sides,
k_rows_append<1..5> by the words per new row, k_rows_append<0> beyond 160 genomes) on rows PLANTED into rows containers
(tests/rows_craft.py) and column blocks written from numpy.  The reference is the numpy model of tests/add_ref.py, held to
the oracle on the CPU (tests/test_add_cpu.py); every comparison is exact.

The source is planted with 0xFF in every byte that is no row byte (contig padding, slack) and, in every second block shape,
with the bits past N_old of its last byte set: neither may reach the destination.  The destination is filled in two source
batches, the second one reading its columns through a pointer into the whole anchor's blocks and their stride, as `add`
does.  About 6 500 positions per case."""
import gzip

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import add_ref as ar
from tests import rows_craft as rc

pytestmark = pytest.mark.gpu

K = 21


def _upload(ctx, arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr)).to(torch.device("cuda", ctx.device))


def _append(ctx, n_old, n_new, per, nparts, gap, stale, fill):
    """the destination after both batches, the model's rows per contig"""
    from panagram_amd import engine
    tile = engine.tile_positions()
    old, new = ar.old_rows(n_old, stale), ar.new_bits(n_old, n_new)
    want = [ar.append_rows(o, n_old, b) for o, b in zip(old, new)]
    blocks, stride = ar.column_blocks(new, nparts, per, tile, gap_words=gap, fill=fill)
    d_blocks = _upload(ctx, blocks)
    dst = rc.container(ctx, K, n_new, ar.NKS)
    try:
        tiles_before = sum((nk + tile - 1) // tile for nk in ar.NKS[:ar.SPLIT])
        for c0, c1, off in ((0, ar.SPLIT, 0), (ar.SPLIT, len(ar.NKS), tiles_before * (tile // 8) * per)):
            src = rc.container(ctx, K, n_old, ar.NKS[c0:c1], colsums=False)
            try:
                rc.plant(src, old[c0:c1], poison=0xFF)
                src.rows_epilogue()  # (finished rows: a container that was never filled is refused as a source)
                dst.append_columns(src, d_blocks.data_ptr() + off, nparts, per, first_contig=c0, part_stride_bytes=stride)
                ctx.synchronize()
            finally:
                src.close()
    except Exception:
        dst.close()
        raise
    return dst, want


@pytest.mark.parametrize("n_old, n_new", ar.WIDTH_PAIRS, ids=[f"{a}to{b}" for a, b in ar.WIDTH_PAIRS])
def test_append_columns_equals_the_model(ctx, n_old, n_new, tmp_path):
    """rows, columns read back out of them (zero beyond every contig's end: the padding stayed clean), the statistics pass
    and the BGZF payload of the appended-to rows, for every block shape that can bring the new genomes"""
    from panagram_amd import engine
    tile = engine.tile_positions()
    shapes = ar.block_shapes(n_old, n_new)
    assert shapes
    for si, (per, nparts, gap) in enumerate(shapes):
        tag = f"{n_old}->{n_new} per {per} nparts {nparts}"
        dst, want = _append(ctx, n_old, n_new, per, nparts, gap, stale=si % 2 == 0, fill=0xFF)
        try:
            cols = _upload(ctx, np.full(dst.columns_bytes(n_new), 0xA5, np.uint8))
            dst.extract_columns(0, n_new, cols.data_ptr())
            ctx.synchronize()
            assert np.array_equal(cols.cpu().numpy(), po.extract_columns(want, n_new, 0, n_new, tile=tile)), tag
            dst.rows_epilogue()
            for ci, (w, nk) in enumerate(zip(want, ar.NKS)):
                rows, low, bins, info = dst.download(ci)
                assert info["nkmers"] == nk, tag
                assert np.array_equal(rows, w), (tag, ci)
                rbins, _, rlow = rc.ref_stats(w, n_new, rc.bin_length(nk), 100)
                assert low.shape == rlow.shape and np.array_equal(low, rlow), (tag, ci)
                assert bins.shape == rbins.shape and np.array_equal(bins.astype(np.int64), rbins), (tag, ci)
            cs = np.stack([rc.ref_stats(w, n_new, rc.bin_length(nk), 100)[1] for w, nk in zip(want, ar.NKS)])
            assert np.array_equal(dst.contig_colsums().astype(np.int64), cs), tag
            if si == 0:
                gz = str(tmp_path / "bitmap.1.gz")
                dst.write_bgzf(1, gz, gz + "i")
                assert gzip.open(gz, "rb").read() == b"".join(w.tobytes() for w in want), tag
        finally:
            dst.close()


def test_mismatched_geometry_is_refused(ctx):
    """a source whose contigs do not have the destination's k-mer counts, too few or too many genomes, a source that is
    the destination: PG_E_INVALID before anything is launched, and the context goes on working"""
    import torch
    from panagram_amd._lib import PanagramHipError
    nks = [100, 1025, 17]
    dst = rc.container(ctx, K, 9, nks)
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=torch.device("cuda", ctx.device))
    bad = [(8, [100, 1024, 17], 0, 1, 1),   # one contig a row short
           (8, [1025, 17], 0, 1, 1),        # right lengths, wrong place
           (8, [100, 1025, 17], 1, 1, 1),   # runs past the destination's contigs
           (7, [100, 1025, 17], 0, 1, 1),   # 7 + 1 genomes are not 9
           (10, [100, 1025, 17], 0, 1, 1),  # more genomes than the destination
           (8, [100, 1025, 17], 0, 0, 1), (8, [100, 1025, 17], 0, 1, 0)]
    try:
        for n_old, src_nks, c0, nparts, per in bad:
            src = rc.container(ctx, K, n_old, src_nks, colsums=False)
            try:
                rc.plant(src, [rc.zeros(nk, n_old) for nk in src_nks])
                src.rows_epilogue()
                with pytest.raises(PanagramHipError) as ei:
                    dst.append_columns(src, buf.data_ptr(), nparts, per, first_contig=c0)
                assert ei.value.code == -1, (n_old, src_nks, c0)  # PG_E_INVALID
            finally:
                src.close()
        with pytest.raises(PanagramHipError):
            dst.append_columns(dst, buf.data_ptr(), 1, 1)
        # the context stays usable: the right call goes through
        src = rc.container(ctx, K, 8, nks, colsums=False)
        try:
            with pytest.raises(PanagramHipError, match="holds no rows"):  # a container nothing has filled or finished
                dst.append_columns(src, buf.data_ptr(), 1, 1)
            rc.plant(src, [rc.ones(nk, 8) for nk in nks])
            src.rows_epilogue()
            dst.append_columns(src, buf.data_ptr(), 1, 1)
            ctx.synchronize()
            for ci, nk in enumerate(nks):
                assert np.array_equal(dst.download(ci, want_bitmap100=False)[0], ar.append_rows(rc.ones(nk, 8), 8, np.zeros((nk, 1))))
        finally:
            src.close()
    finally:
        dst.close()
