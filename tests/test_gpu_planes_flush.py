"""GPU: the flush of the column sums' counter planes (panagram_amd/csrc/pg_planes.h) in the MIDDLE of a contig — the transposition
into byte counters, the halving exchange over the wave, the zeroing of the planes, the reset of `vrows`, the carries held back
at a flush that comes at 248 or 252 rows — in every statistics kernel of pg_rows.hip that has one:
  k_epilogue_n<2..8>   group path and one windowed tile, after 240 rows of a thread (its own wording of the flush)
  k_epilogue_w<9..16>  at the top of the tile loop, once another group would not fit: 248 rows, or 252 where groups and single
                       tiles come in turn
  k_epilogue_chunks    <2, false> (N = 130) and <2, true> (N = 256), after 240 rows of a lane
and one-byte rows (N = 8: k_epilogue_b1, accumulators of its own) under the same launches.

A launch of the default shape gives a workgroup about 16 tiles (64 rows per thread) until it holds more than 16 384 tiles, so
at test sizes none of these lines runs for rows of 2..16 bytes.  PG_EPI_WORKGROUPS — a test switch of launch_rows_epilogue,
read at every launch — bounds the grid: with 1 one workgroup walks every contig, with 2 a second one starts at tile 35 of the
long contig and still has 97 of its tiles.  Which thread then meets which flush, with how many rows in its planes, is
restated in tests/epi_walk.py and held to these cases on the CPU (tests/test_rows_craft_cpu.py).

The rows (tests/rows_craft.py, flush_rows): a contig of exactly 60 tiles of ones and a partial tile; a contig of 131 tiles and a
partial one whose first 64 tiles are rows of all N bits — every column of every thread stands at 240 (248, 252) when the
first flush comes — followed by ramp, bursts of 255 / 256 / 257, the last column alone and dense rows; a short contig behind.
Bins, column sums, low-resolution rows and the rows themselves equal rc.ref_stats exactly under both bounds, and the launch
of the default shape over the same container gives the same.  On an MI355X the 57 cases take 0.04 to 0.08 s each, the file 3 s
(run alone 15 s: the first case pays the 12 s in which the process loads the library's code objects).

With the flush of one site disabled in a scratch build (the planes wrap: wrong sums, no fault) exactly that site's cases fail
here — n.group: N 13..61 default and long_bins; n.tile: N 13..61 one_tile; k_epilogue_w: N 72..128, every geometry;
k_epilogue_chunks: N 130 and 256 — while tests/test_gpu_rows_craft.py passes for the first three and, for the chunk kernel,
fails only from three chunks per row on (N = 300 and wider), whose lanes take 16 rows and more per tile."""
import numpy as np
import pytest

from tests import rows_craft as rc

pytestmark = pytest.mark.gpu

K = 21
ENV = "PG_EPI_WORKGROUPS"
_cache = {"rows": (None, None), "ref": (None, None)}


def _rows(n):
    if _cache["rows"][0] != n:
        _cache["rows"] = (n, rc.flush_rows(n))
    return _cache["rows"][1]


def _reference(n, binlens):
    """rc.ref_stats of every contig, once per N and bin lengths (the cases come N by N, geometry by geometry)"""
    key = (n, tuple(binlens))
    if _cache["ref"][0] != key:
        _cache["ref"] = (key, [rc.ref_stats(r, n, bl, 100) for r, bl in zip(_rows(n), binlens)])
    return _cache["ref"][1]


def _outputs(res, want_cs):
    from panagram_amd._lib import PanagramHipError
    out = [res.download(ci) for ci in range(len(res.seqs.lens))]
    if want_cs:
        return out, res.contig_colsums()
    with pytest.raises(PanagramHipError, match="PG_ANCHOR_COLSUMS"):  # column sums that were not asked for are refused
        res.contig_colsums()
    return out, None


def _run_bounds(ctx, monkeypatch, n, geometry, poison=None):
    """plant the flush rows once; the statistics pass under every bound and, last, with the variable unset: {bound: outputs}"""
    res = rc.container(ctx, K, n, rc.FLUSH_NK, **geometry)
    want_cs = geometry.get("colsums", True)
    outs = {}
    try:
        rc.plant(res, _rows(n), poison=poison)
        for bound in rc.FLUSH_BOUNDS + [None]:
            if bound is None:
                monkeypatch.delenv(ENV, raising=False)
            else:
                monkeypatch.setenv(ENV, str(bound))
            res.rows_epilogue()
            outs[bound] = _outputs(res, want_cs)
    finally:
        res.close()
    return outs


def _hold(n, geometry, outs, tag):
    """every output of every launch shape equals the reference — hence the bounded runs equal the default-shaped one"""
    want_cs = geometry.get("colsums", True)
    binlens = [rc.bin_length(nk, geometry.get("max_bin_len", 200000), geometry.get("min_bin_count", 100)) for nk in rc.FLUSH_NK]
    ref = _reference(n, binlens)
    for bound, (out, got_cs) in outs.items():
        for ci, (r, nk) in enumerate(zip(_rows(n), rc.FLUSH_NK)):
            t = f"N {n} {tag} bound {bound} contig {ci} ({nk} rows)"
            got_rows, got_low, got_bins, info = out[ci]
            bins, cs, low = ref[ci]
            assert info["nkmers"] == nk and info["binlen"] == binlens[ci], t
            assert np.array_equal(got_rows, r), t
            assert got_low.shape == low.shape and np.array_equal(got_low, low), t
            assert got_bins.shape == bins.shape and np.array_equal(got_bins.astype(np.int64), bins), t
            if want_cs:
                got = got_cs[ci].astype(np.int64)
                assert np.array_equal(got, cs), f"{t}: column sums off by {(got - cs).tolist()}"
            else:
                assert got_cs is None, t
    free, free_cs = outs[None]  # agreement with the default shape, output by output
    for bound in rc.FLUSH_BOUNDS:
        out, got_cs = outs[bound]
        assert (got_cs is None and free_cs is None) or np.array_equal(got_cs, free_cs), (tag, bound)
        for x, y in zip(out, free):
            assert all(np.array_equal(p, q) for p, q in zip(x[:3], y[:3])) and x[3] == y[3], (tag, bound)


@pytest.mark.parametrize("n, geom", rc.flush_cases(), ids=[f"N{n}_{g}" for n, g in rc.flush_cases()])
def test_planes_flush_in_mid_contig(ctx, monkeypatch, n, geom):
    """one and two workgroups over contigs of 60, 131 and 2 full tiles and a partial one each: every mid-contig flush site of the
    width's kernel runs at least twice inside one contig, with rows behind the last flush (tests/test_rows_craft_cpu.py says
    which geometry reaches which site), and all outputs equal the reference and the default-shaped launch's"""
    geometry = rc.flush_geometries(n)[geom]
    _hold(n, geometry, _run_bounds(ctx, monkeypatch, n, geometry), geom)


@pytest.mark.parametrize("n", [8, 13, 77, 130])
def test_planes_flush_ignores_bytes_outside_the_rows(ctx, monkeypatch, n):
    """one width of each kernel once more with 0xFF in every byte of the row buffer that is no row byte"""
    _hold(n, {}, _run_bounds(ctx, monkeypatch, n, {}, poison=0xFF), "poison 0xFF")


@pytest.mark.parametrize("n", [29, 104, 130])
def test_bounded_launch_without_column_sums(ctx, monkeypatch, n):
    """colsums=False under the bound, everything else equal: the planes stay empty, bins, low-resolution rows and rows equal the
    reference, and column sums are refused as in a launch of the default shape"""
    geometry = dict(colsums=False)
    _hold(n, geometry, _run_bounds(ctx, monkeypatch, n, geometry), "no column sums")
