"""GPU: selecting columns out of finished rows (AnchorResult.select_columns: k_rows_select_b1 for one-byte rows on both
sides, k_rows_select<1..5> by the words per source row, k_rows_select<0> beyond 160 genomes) on rows PLANTED into rows
containers (tests/rows_craft.py).  The reference is the numpy model of tests/subset_ref.py, held to the oracle on the CPU
(tests/test_subset_cpu.py); every comparison is exact.

The source is planted with 0xFF in every byte that is no row byte (contig padding, slack) and, in every second selection,
with the bits past N_old of its last byte set: neither may reach the destination.  The destination is filled in two source
batches, split at contig 7, as `subset` fills it.  About 6 500 positions per case."""
import gzip

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import rows_craft as rc
from tests import subset_ref as sr

pytestmark = pytest.mark.gpu

K = 21
BATCHES = ((0, sr.SPLIT), (sr.SPLIT, len(sr.NKS)))


def _upload(ctx, arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr)).to(torch.device("cuda", ctx.device))


class _Sources:
    """the planted source batches of one N_old, with and without stale bits: planted once, read by every selection"""

    def __init__(self, ctx, n_old):
        self.rows = {stale: sr.old_rows(n_old, stale) for stale in (False, True)}
        self.res = {}
        try:
            for stale, rows in self.rows.items():
                for c0, c1 in BATCHES:
                    src = self.res[stale, c0] = rc.container(ctx, K, n_old, sr.NKS[c0:c1], colsums=False)
                    rc.plant(src, rows[c0:c1], poison=0xFF)
                    src.rows_epilogue()  # (finished rows: a container that was never filled is refused as a source)
            ctx.synchronize()
        except Exception:
            self.close()
            raise

    def close(self):
        for r in self.res.values():
            r.close()
        self.res = {}


def _select(ctx, srcs, sel, stale):
    """a destination of len(sel) genomes after both batches"""
    dst = rc.container(ctx, K, len(sel), sr.NKS)
    try:
        for c0, _ in BATCHES:
            dst.select_columns(srcs.res[stale, c0], sel, first_contig=c0)
        ctx.synchronize()
    except Exception:
        dst.close()
        raise
    return dst


@pytest.mark.parametrize("n_old, n_new", sr.WIDTH_PAIRS, ids=[f"{a}to{b}" for a, b in sr.WIDTH_PAIRS])
def test_select_columns_equals_the_model(ctx, n_old, n_new, tmp_path):
    """rows, columns read back out of them (zero beyond every contig's end: the padding stayed clean), the statistics pass
    and the BGZF payload of the selected rows, for every selection of the pair"""
    from panagram_amd import engine
    tile = engine.tile_positions()
    srcs = _Sources(ctx, n_old)
    try:
        for si, (name, sel) in enumerate(sr.selections(n_old, n_new)):
            tag = f"{n_old}->{len(sel)} {name}"
            n = len(sel)
            want = [sr.select_rows(o, n_old, sel) for o in srcs.rows[False]]
            dst = _select(ctx, srcs, sel, stale=si % 2 == 1)
            try:
                cols = _upload(ctx, np.full(dst.columns_bytes(n), 0xA5, np.uint8))
                dst.extract_columns(0, n, cols.data_ptr())
                ctx.synchronize()
                assert np.array_equal(cols.cpu().numpy(), po.extract_columns(want, n, 0, n, tile=tile)), tag
                dst.rows_epilogue()
                for ci, (w, nk) in enumerate(zip(want, sr.NKS)):
                    rows, low, bins, info = dst.download(ci)
                    assert info["nkmers"] == nk, tag
                    assert np.array_equal(rows, w), (tag, ci)
                    rbins, _, rlow = rc.ref_stats(w, n, rc.bin_length(nk), 100)
                    assert low.shape == rlow.shape and np.array_equal(low, rlow), (tag, ci)
                    assert bins.shape == rbins.shape and np.array_equal(bins.astype(np.int64), rbins), (tag, ci)
                cs = np.stack([rc.ref_stats(w, n, rc.bin_length(nk), 100)[1] for w, nk in zip(want, sr.NKS)])
                assert np.array_equal(dst.contig_colsums().astype(np.int64), cs), tag
                if name == "middle":
                    gz = str(tmp_path / "bitmap.1.gz")
                    dst.write_bgzf(1, gz, gz + "i")
                    assert gzip.open(gz, "rb").read() == b"".join(w.tobytes() for w in want), tag
            finally:
                dst.close()
    finally:
        srcs.close()


@pytest.mark.parametrize("n_old, n_new", [(9, 8), (65, 64), (64, 8), (170, 161)], ids=lambda v: str(v))
def test_select_columns_equals_extract_and_merge(ctx, n_old, n_new):
    """the one pass and the composition that was there before it — one extract_columns(g, 1) per kept genome into block i,
    then merge_columns_range(per=1) — leave the same rows"""
    import torch
    srcs = _Sources(ctx, n_old)
    try:
        for name, sel in sr.selections(n_old, n_new):
            if name not in ("middle", "shuffle"):
                continue
            fused = _select(ctx, srcs, sel, stale=False)
            comp = rc.container(ctx, K, n_new, sr.NKS)
            try:
                for c0, c1 in BATCHES:
                    src = srcs.res[False, c0]
                    block = src.columns_bytes(1)
                    cols = torch.empty(max(8, block * n_new), dtype=torch.uint8, device=torch.device("cuda", ctx.device))
                    for i, g in enumerate(sel):
                        src.extract_columns(int(g), 1, cols.data_ptr() + i * block)
                    comp.merge_columns_range(cols.data_ptr(), 0, n_new, 1, c0, c1 - c0)
                    ctx.synchronize()
                assert torch.equal(fused.rows_tensor(), comp.rows_tensor()), (n_old, n_new, name)
            finally:
                fused.close()
                comp.close()
    finally:
        srcs.close()


def test_bad_selections_and_geometry_are_refused(ctx):
    """every refusal: PG_E_INVALID before anything is launched; then the right call goes through on the same context"""
    from panagram_amd._lib import PanagramHipError
    nks = [100, 1025, 17]
    dst = rc.container(ctx, K, 8, nks)
    ok = list(range(8))
    bad = [(9, nks, 0, list(range(7))),            # nsel != the destination's genomes
           (9, nks, 0, list(range(9))),
           (9, nks, 0, [0, 1, 2, 3, 4, 5, 6, 9]),  # an entry >= N_old
           (9, nks, 0, [0, 1, 2, 3, 4, 5, 6, 6]),  # a duplicate
           (9, nks, 0, []),                        # nothing selected
           (9, [100, 1024, 17], 0, ok),           # one contig a row short
           (9, [1025, 17], 0, ok),                 # right lengths, wrong place
           (9, nks, 1, ok)]                        # runs past the destination's contigs
    try:
        for n_old, src_nks, c0, sel in bad:
            src = rc.container(ctx, K, n_old, src_nks, colsums=False)
            try:
                rc.plant(src, [rc.zeros(nk, n_old) for nk in src_nks])
                src.rows_epilogue()
                with pytest.raises(PanagramHipError) as ei:
                    dst.select_columns(src, sel, first_contig=c0)
                assert ei.value.code == -1, (n_old, src_nks, c0, sel)  # PG_E_INVALID
            finally:
                src.close()
        with pytest.raises(PanagramHipError) as ei:
            dst.select_columns(dst, ok)
        assert ei.value.code == -1
        src = rc.container(ctx, K, 9, nks, colsums=False)
        try:
            with pytest.raises(PanagramHipError, match="holds no rows") as ei:  # a container nothing has filled or finished
                dst.select_columns(src, ok)
            assert ei.value.code == -1
            # the context stays usable: the right call goes through
            old = [rc.dense(nk, 9, 7 + i) for i, nk in enumerate(nks)]
            rc.plant(src, old)
            src.rows_epilogue()
            sel = [8, 0, 1, 2, 3, 5, 6, 7]
            dst.select_columns(src, sel)
            ctx.synchronize()
            for ci, o in enumerate(old):
                assert np.array_equal(dst.download(ci, want_bitmap100=False)[0], sr.select_rows(o, 9, sel))
        finally:
            src.close()
    finally:
        dst.close()
