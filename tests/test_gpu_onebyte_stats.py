"""The statistics pass over one-byte rows (k_epilogue_b1, N <= 8 genomes) against the oracle: bitmap.100 rows, bins
and per-contig column sums, for every path the pass takes — whole one-bin groups (streaks), groups across several short
bins, bins shorter than a tile (the per-tile path), contigs that end inside a group, thousands of contigs of less than a
tile (a workgroup's range crosses many of them), a run in chunks (PG_RUN_CHUNKS: launches over tile ranges), column sums
off, and a low-resolution step other than 100 (k_lowres takes the rows).  Bit-exact, as everywhere."""
import numpy as np
import pytest

from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

GROUP = 8 * 1024  # rows of one group of the pass (8 tiles)


def _bins_of(popc, n, binlen):
    nb = (len(popc) + binlen - 1) // binlen
    out = np.zeros((nb, n + 1), np.int64)
    for b in range(nb):
        out[b] = np.bincount(popc[b * binlen:(b + 1) * binlen], minlength=n + 1)[:n + 1]
    return out


def _binlen(nk, max_bin, min_count):
    b = max_bin if nk // max_bin >= min_count else nk // min_count
    return max(b, 1)


@pytest.mark.parametrize("n", [1, 3, 7, 8])
def test_one_byte_statistics_every_path_against_oracle(ctx, n, monkeypatch):
    from panagram_amd import engine
    k = 21
    rng = np.random.default_rng(70 + n)
    lens = [400_000 + 777,                      # long: streaks of whole one-bin groups (bins of 50 000 rows), a ragged end
            5 * GROUP + 3_333 + k - 1,          # ends inside a group
            3 * GROUP + k - 1,                  # exactly three groups
            5_000, 3_100, 1_500]                # a few kb: bins shorter than a tile
    lens += [int(x) for x in rng.integers(150, 900, 1500)]  # many contigs of less than a tile
    gen = po.synth_genomes(n, lens, 0.02, 900 + n)
    genomes = [[bytearray(po.codes_to_ascii(c)) for c in g] for g in gen]
    for g in range(n):  # N runs (rows of zeros) and lower case in the long contig
        c = genomes[g][0]
        p = int(rng.integers(0, len(c) - 3000))
        c[p:p + 2500] = b"N" * 2500
        q = int(rng.integers(0, len(c) - 500))
        c[q:q + 400] = bytes(c[q:q + 400]).lower()
    genomes = [[bytes(c) for c in g] for g in genomes]
    dbs = po.build_bitvec_dbs(genomes, k)
    tbl = engine.PanTable(ctx, k, n)
    for g in range(n):
        ss = engine.SeqSet.from_host(ctx, genomes[g])
        tbl.insert_seqset(g, ss)
        ss.close()
    ga = n - 1
    oracle = []
    for seq in genomes[ga]:
        o_rows, _, _, _, o_cs = po.anchor_contig(dbs, seq, k, n)
        popc = np.minimum(np.unpackbits(o_rows, axis=1).sum(axis=1, dtype=np.int64), n)
        oracle.append((o_rows, popc, o_cs))
    ss = engine.SeqSet.from_host(ctx, genomes[ga])

    def check(tag, colsums=True, step=100, max_bin=200_000, min_count=100, chunks=None):
        if chunks:
            monkeypatch.setenv("PG_RUN_CHUNKS", str(chunks))
            monkeypatch.setenv("PG_CHUNK_MIN_TILES", "4")
        res = engine.AnchorResult(tbl, ss, colsums=colsums, lowres_step=step, max_bin_len=max_bin, min_bin_count=min_count)
        res.run()
        res.run()  # (a second run over the same result: the statistics start from zero again)
        ccs = res.contig_colsums().astype(np.int64) if colsums else None
        for ci, (o_rows, popc, o_cs) in enumerate(oracle):
            rows, rows_lo, bins, info = res.download(ci)
            nk = len(o_rows)
            bl = _binlen(nk, max_bin, min_count)
            assert info["binlen"] == bl and info["nkmers"] == nk, (tag, ci)
            assert np.array_equal(rows, o_rows), (tag, ci)
            assert np.array_equal(rows_lo, o_rows[::step]), (tag, ci)
            assert np.array_equal(bins.astype(np.int64), _bins_of(popc, n, bl)), (tag, ci)
            if colsums:
                assert np.array_equal(ccs[ci], o_cs), (tag, ci)
        res.close()
        if chunks:
            monkeypatch.delenv("PG_RUN_CHUNKS")
            monkeypatch.delenv("PG_CHUNK_MIN_TILES")

    check("default bins")                                  # bins of nkmers / 100 rows: groups across short bins, per-tile path
    check("long bins", max_bin=50_000, min_count=1)        # the long contig in bins of 50 000 rows: streaks
    check("no colsums, lowres 7", colsums=False, step=7)
    check("chunks", chunks=3, max_bin=50_000, min_count=1)
    ss.close()
    tbl.close()
